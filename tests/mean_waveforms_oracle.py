"""Test-only restatements of mts_mean_waveforms in numpy: the definition of include/mtscomp_hip.h twice -- vectorised (on the snippets
of tests/waveforms_oracle.py, np.rint and np.add.at) and by brute force (every entry visited in plain loops, the rounding spelt
out) -- and a lane codec built on the first so that the CPU suite drives Reader.mean_waveforms (argument handling, order, labels,
calls, lanes, cache use, errors) and can check identity."""
import math

import numpy as np

from tests.waveforms_oracle import WaveformsOracleCodec, reference_rows, waveforms

LIMIT = 2.0 ** 42


def mean_waveforms(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, ev_label, n_labels, before, after, width, resolution):
    """(sum int64 (n_labels, T, width), count int32 (n_labels, T, width), skipped int64 (n_labels)).  x: the selected columns of file
    rows [x_row0, x_row0 + len(x)), any item type; [vb, ve): the recording; reference 0 / 1; ev_row any order."""
    ev_row, ev_col0, ev_label = (np.asarray(a, dtype=np.int64) for a in (ev_row, ev_col0, ev_label))
    n, T, n_cols = ev_row.size, before + after, x.shape[1]
    total, count, skipped = np.zeros((n_labels, T, width), np.int64), np.zeros((n_labels, T, width), np.int32), np.zeros(n_labels, np.int64)
    if not n:
        return total, count, skipped
    assert (ev_label >= 0).all() and (ev_label < n_labels).all()
    wave = waveforms(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width)[0]
    r = ev_row[:, None, None] - before + np.arange(T)[None, :, None]
    c = ev_col0[:, None, None] + np.arange(width)[None, None, :]
    inside = np.broadcast_to((r >= vb) & (r < ve) & (c >= 0) & (c < n_cols), wave.shape)     # (a NaN elsewhere is a fill entry: nothing)
    with np.errstate(over='ignore', invalid='ignore'):
        d = wave.astype(np.float64) * (1.0 / resolution)
        good = inside & (np.abs(d) < LIMIT)                              # (False for a NaN)
    e, tau, w = np.nonzero(good)
    np.add.at(total, (ev_label[e], tau, w), np.rint(d[good]).astype(np.int64))
    np.add.at(count, (ev_label[e], tau, w), 1)
    np.add.at(skipped, ev_label[np.nonzero(inside & ~good)[0]], 1)
    return total, count, skipped


# ---- the same definition by brute force: every entry in plain loops, half-to-even spelt out ----------------------------------------
def rint_half_even(d):
    f = math.floor(d)
    diff = d - f                                                         # (exact: |d| < 2^42, so d has fraction bits to spare)
    if diff > 0.5 or (diff == 0.5 and f % 2):
        f += 1
    return int(f)


def mean_waveforms_brute(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, ev_label, n_labels, before, after, width, resolution):
    T, n_cols = before + after, x.shape[1]
    total, count, skipped = np.zeros((n_labels, T, width), np.int64), np.zeros((n_labels, T, width), np.int32), np.zeros(n_labels, np.int64)
    for e in range(len(ev_row)):
        s, c0, l = int(ev_row[e]), int(ev_col0[e]), int(ev_label[e])
        a, b = max(vb, s - before), min(ve, s + after)
        z = reference_rows(x, x_row0, vb, ve, a, b, taps, reference) if a < b else None
        for tau in range(T):
            for w in range(width):
                r, c = s - before + tau, c0 + w
                if not (vb <= r < ve and 0 <= c < n_cols):
                    continue
                d = float(z[r - a, c]) / resolution
                if math.isnan(d) or abs(d) >= LIMIT:
                    skipped[l] += 1
                    continue
                total[l, tau, w] += rint_half_even(d)
                count[l, tau, w] += 1
    return total, count, skipped


def mean_of(total, count, resolution):
    """Reader.mean_waveforms' mean from its sums."""
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = (total.astype(np.float64) * resolution / count).astype(np.float32)
    mean[count == 0] = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]
    return mean


class MeanWaveformsOracleCodec(WaveformsOracleCodec):
    """WaveformsOracleCodec + mean_waveforms restated in numpy, chunks read as waveforms reads them.  Records (lane, keys, lens,
    n_events) of every mean_waveforms call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.mean_waveforms_calls = []
        self.miss_next_mean_waveforms = False        # simulate an entry dropped between the query and the call

    def mean_waveforms(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols,
                       reference, ev_row, ev_col0, ev_label, n_labels, before, after, width, resolution, lane=None):
        ev_row, ev_col0, ev_label = (np.asarray(a, dtype=np.int64) for a in (ev_row, ev_col0, ev_label))
        self.mean_waveforms_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(ev_row.size)))
        cols = np.asarray(cols, dtype=np.int64)
        taps = np.asarray(taps, dtype=np.float64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all() and reference in (0, 1)
        assert before >= 0 and after >= 0 and 1 <= before + after <= 4096 and 1 <= width <= 1024
        assert 1 <= n_labels <= 4096 and n_labels * (before + after) * width <= 1 << 27
        assert math.frexp(resolution)[0] == 0.5 and -60 <= math.frexp(resolution)[1] - 1 <= 60
        assert ev_row.size and (np.diff(ev_row) >= 0).all() and valid_begin <= ev_row[0] and ev_row[-1] < valid_end, 'events'
        assert ev_label.shape == ev_row.shape and (ev_label >= 0).all() and (ev_label < n_labels).all(), 'labels'
        assert np.bincount(ev_label).max() <= 1 << 21
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        half = (taps.size - 1) // 2
        lo, hi = max(valid_begin, int(ev_row[0]) - before + half - (taps.size - 1)), min(valid_end, int(ev_row[-1]) + after + half)
        assert int(row0[0]) <= lo and hi <= int(row0[-1]) + int(n_rows[-1]), 'the chunks do not cover the rows read'
        status, arrays = self._call_chunks('mean_waveforms', cache_id, keys, cdata, offs, lens, n_rows, n_channels, np.dtype(dtype), flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        return (status,) + mean_waveforms(x, int(row0[0]), valid_begin, valid_end, taps, reference, ev_row, ev_col0, ev_label, n_labels, before,
                                          after, width, resolution)
