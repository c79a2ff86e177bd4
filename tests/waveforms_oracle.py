"""Test-only restatements of mts_waveforms in numpy: the definition of include/mtscomp_hip.h twice -- vectorised (on the filter and
the median of tests/detect_oracle.py, one fancy index for the gather, nanargmin-style reductions) and by brute force (every entry
built and compared in plain loops) -- and a lane codec built on the first so that the CPU suite drives Reader.waveforms (argument
handling, order, calls, lanes, cache use, errors) and can check bit-identity."""
import math

import numpy as np

from tests.codec_oracle import LaneOracleCodec
from tests.detect_oracle import filtered, row_median

FILL = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]


def reference_rows(x, x_row0, vb, ve, a, b, taps, reference):
    """z (float32) for file rows [a, b): detect's z."""
    z = filtered(x, x_row0, vb, ve, a, b, np.asarray(taps, dtype=np.float64))
    if reference:
        with np.errstate(invalid='ignore', over='ignore'):
            z = (z - row_median(z)[:, None]).astype(np.float32)
    return z


def extrema(wave):
    """(min, argmin, max, argmax) of every snippet of wave (n, T, W) over the entries that are not NaN: the first in (tau, w) order,
    -0 == +0, its own bits; (NaN, -1) for none."""
    n = wave.shape[0]
    flat = wave.reshape(n, wave.shape[1] * wave.shape[2])
    some = ~np.isnan(flat)
    out = []
    for worst, arg in ((np.inf, np.argmin), (-np.inf, np.argmax)):
        idx = arg(np.where(some, flat, np.float32(worst)), axis=1).astype(np.int64)     # (the first of equal values)
        # an entry equal to the stand-in (+-inf itself) must not lose to a NaN before it
        idx = np.where(some[np.arange(n), idx], idx, np.argmax(some, axis=1))
        val = flat[np.arange(n), idx].copy()
        none = ~some.any(axis=1)
        val[none] = FILL
        idx[none] = -1
        out += [val.astype(np.float32), idx]
    return tuple(out)


def waveforms(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width):
    """(wave float32 (n, T, width), min, argmin int64, max, argmax int64).  Every NaN entry, fill or data, has the bits of FILL.  x: the selected columns of file rows [x_row0, x_row0 +
    len(x)), any item type; [vb, ve): the recording; reference 0 / 1; ev_row any order."""
    ev_row, ev_col0 = np.asarray(ev_row, dtype=np.int64), np.asarray(ev_col0, dtype=np.int64)
    n, T, n_cols = ev_row.size, before + after, x.shape[1]
    wave = np.full((n, T, width), FILL, np.float32)
    if n:
        a, b = max(vb, int(ev_row.min()) - before), min(ve, int(ev_row.max()) + after)
        z = reference_rows(x, x_row0, vb, ve, a, b, taps, reference)
        r = ev_row[:, None, None] - before + np.arange(T)[None, :, None]
        c = ev_col0[:, None, None] + np.arange(width)[None, None, :]
        ok = (r >= vb) & (r < ve) & (c >= 0) & (c < n_cols)
        r, c = np.broadcast_arrays(r, c)
        wave[ok] = z[r[ok] - a, c[ok]]
        wave[np.isnan(wave)] = FILL                                      # (a NaN of the data: the same bits as the fill)
    return (wave,) + extrema(wave)


# ---- the same definition by brute force: every entry and every comparison in plain loops -----------------------------------------
def waveforms_brute(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width):
    n, T, n_cols = len(ev_row), before + after, x.shape[1]
    wave = np.full((n, T, width), FILL, np.float32)
    vmin, vmax = np.full(n, FILL, np.float32), np.full(n, FILL, np.float32)
    amin, amax = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for e in range(n):
        s, c0 = int(ev_row[e]), int(ev_col0[e])
        a, b = max(vb, s - before), min(ve, s + after)
        z = reference_rows(x, x_row0, vb, ve, a, b, taps, reference) if a < b else None
        for tau in range(T):
            for w in range(width):
                r, c = s - before + tau, c0 + w
                if not (vb <= r < ve and 0 <= c < n_cols):
                    continue
                v = z[r - a, c]
                if math.isnan(v):                                        # (stored as the fill's bits)
                    continue
                wave[e, tau, w] = v
                if amin[e] < 0 or v < vmin[e]:
                    vmin[e], amin[e] = v, tau * width + w
                if amax[e] < 0 or v > vmax[e]:
                    vmax[e], amax[e] = v, tau * width + w
    return wave, vmin, amin, vmax, amax


class WaveformsOracleCodec(LaneOracleCodec):
    """LaneOracleCodec + detect (for the events of the tests) and waveforms restated in numpy: resident chunks read from the lane's
    cache dict (E_MISS when a chunk without bytes is not there), the others decoded and NOT inserted.  Records (lane, keys, lens,
    n_events) of every waveforms call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.waveforms_calls = []
        self.miss_next_waveforms = False             # simulate an entry dropped between the query and the call

    def detect(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end,
               taps, cols, threshold, sign, reference, exclude_rows, exclude_cols, max_events, lane=None):
        from tests.detect_oracle import detect_events
        status, arrays = self._call_chunks('detect', cache_id, keys, cdata, offs, lens, n_rows, n_channels, np.dtype(dtype), flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, np.asarray(cols, dtype=np.int64)]
        row, pos, amp = detect_events(x, int(row0[0]), valid_begin, valid_end, row_begin, row_end, taps, threshold, sign, reference,
                                      exclude_rows, exclude_cols)
        k = min(row.size, int(max_events))
        return status, int(row.size), row[:k], pos[:k].astype(np.int32), amp[:k]

    def waveforms(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols,
                  reference, ev_row, ev_col0, before, after, width, want_wave=True, lane=None):
        ev_row, ev_col0 = np.asarray(ev_row, dtype=np.int64), np.asarray(ev_col0, dtype=np.int64)
        self.waveforms_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(ev_row.size)))
        cols = np.asarray(cols, dtype=np.int64)
        taps = np.asarray(taps, dtype=np.float64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all() and reference in (0, 1)
        assert before >= 0 and after >= 0 and 1 <= before + after <= 4096 and 1 <= width <= 1024
        assert ev_row.size and (np.diff(ev_row) >= 0).all() and valid_begin <= ev_row[0] and ev_row[-1] < valid_end, 'events'
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        half = (taps.size - 1) // 2
        lo, hi = max(valid_begin, int(ev_row[0]) - before + half - (taps.size - 1)), min(valid_end, int(ev_row[-1]) + after + half)
        assert int(row0[0]) <= lo and hi <= int(row0[-1]) + int(n_rows[-1]), 'the chunks do not cover the rows read'
        status, arrays = self._call_chunks('waveforms', cache_id, keys, cdata, offs, lens, n_rows, n_channels, np.dtype(dtype), flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        wave, vmin, amin, vmax, amax = waveforms(x, int(row0[0]), valid_begin, valid_end, taps, reference, ev_row, ev_col0, before, after, width)
        return status, (wave if want_wave else None), vmin, amin.astype(np.int32), vmax, amax.astype(np.int32)


# ---- the base case of the suites: synth_int16(0, 3000, 70, 4) through 65 high-pass taps, the events of detect(12, exclude=7,
# spread=3, sign='neg'), 20 rows before and 41 after, 8 neighbours either side
BASE_COUNTS = {0: dict(events=371, clip_lo=2, clip_hi=6, clip_left=41, clip_right=30, repeats=18),
               1: dict(events=397, clip_lo=2, clip_hi=7, clip_left=46, clip_right=37, repeats=17)}


def edge_counts(sample, col0, before, after, width, n_rows, n_cols):
    """How many events reach each edge: so that no test reaches one vacuously."""
    sample, col0 = np.asarray(sample), np.asarray(col0)
    return dict(events=int(sample.size), clip_lo=int((sample < before).sum()), clip_hi=int((sample + after > n_rows).sum()),
                clip_left=int((col0 < 0).sum()), clip_right=int((col0 + width > n_cols).sum()),
                repeats=int(sample.size - np.unique(sample).size))
