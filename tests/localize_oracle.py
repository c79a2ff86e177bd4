"""Test-only restatements of mts_localize in numpy: the definition of include/mtscomp_hip.h twice -- vectorised (the snippets of
tests/waveforms_oracle.py, arg-reductions for the column extrema, one exact fmaf over all events per position) and by brute force
(scalar loops over every entry, libm's fmaf) -- and a lane codec built on the first so that the CPU suite drives Reader.localize
(argument handling, order, calls, lanes, cache use, errors) and can check bit-identity."""
import math

import numpy as np

from tests.correlate_oracle import _libm_fmaf
from tests.project_oracle import fmaf_f32
from tests.waveforms_oracle import FILL, WaveformsOracleCodec, waveforms

MAX_DIMS = 4
MODES = {'ptp': 0, 'neg': 1, 'pos': 2, 'abs': 3}


def positions32(positions, n_cols):
    """The positions as the call takes them: float32 (n_cols, D), 1 <= D <= 4, every entry finite."""
    p = np.ascontiguousarray(np.asarray(positions, dtype=np.float32))
    assert p.ndim == 2 and p.shape[0] == n_cols and 1 <= p.shape[1] <= MAX_DIMS and np.isfinite(p).all()
    return p


def _first(arr, some, worst, arg):
    """The first extreme entry (argmin / argmax with the stand-in `worst` for the masked ones) of every column (e, ., w), its own bits."""
    idx = arg(np.where(some, arr, np.float32(worst)), axis=1)            # (n, W): the first of equal values
    # an entry equal to the stand-in (+-inf itself) must not lose to a masked one before it
    idx = np.where(np.take_along_axis(some, idx[:, None, :], axis=1)[:, 0], idx, np.argmax(some, axis=1))
    return np.take_along_axis(arr, idx[:, None, :], axis=1)[:, 0]


def amplitudes(wave, mode):
    """a (n, W) float32 of snippets wave (n, T, W): steps 1 and 2 of the definition."""
    wave = np.asarray(wave, dtype=np.float32)
    some = ~np.isnan(wave)
    with np.errstate(invalid='ignore', over='ignore'):
        if mode == 0:
            a = _first(wave, some, -np.inf, np.argmax) - _first(wave, some, np.inf, np.argmin)
        elif mode == 1:
            a = np.negative(_first(wave, some, np.inf, np.argmin))
        elif mode == 2:
            a = _first(wave, some, -np.inf, np.argmax)
        else:
            assert mode == 3
            a = _first(np.abs(wave), some, -np.inf, np.argmax)
    a = a.astype(np.float32)
    a[~some.any(axis=1) | np.isnan(a)] = FILL
    return a


def chains(a, col0, positions, skip_zero=False):
    """(weight (n), moment (n, D), best (n) int64) of amplitudes a (n, W): steps 3 to 5.  skip_zero: the steps with g = +0 are not
    taken (the same bytes: held in tests/test_localize_oracles.py)."""
    a, col0 = np.asarray(a, dtype=np.float32), np.asarray(col0, dtype=np.int64)
    n, W = a.shape
    n_cols, D = positions.shape
    g = np.where(a > 0, a, np.float32(0.0)).astype(np.float32)
    weight, moment = np.zeros(n, np.float32), np.zeros((n, D), np.float32)
    for w in range(W):
        c = col0 + w
        take = (c >= 0) & (c < n_cols)
        if skip_zero:
            take &= g[:, w] > 0
        with np.errstate(invalid='ignore', over='ignore'):
            weight = np.where(take, weight + g[:, w], weight).astype(np.float32)
        moment = np.where(take[:, None], fmaf_f32(g[:, w, None], positions[np.clip(c, 0, n_cols - 1)], moment), moment).astype(np.float32)
    weight[np.isnan(weight)] = FILL
    moment[np.isnan(moment)] = FILL
    some = ~np.isnan(a)
    best = np.argmax(np.where(some, a, np.float32(-np.inf)), axis=1).astype(np.int64)      # (the first of equal values)
    best = np.where(some[np.arange(n), best], best, np.argmax(some, axis=1))
    best[~some.any(axis=1)] = -1
    return weight, moment, best


def reduce_snippets(wave, col0, positions, mode, skip_zero=False):
    """(amplitude, weight, moment, best) of snippets wave (n, T, W) whose first column positions are col0."""
    a = amplitudes(wave, mode)
    return (a,) + chains(a, col0, positions, skip_zero)


def localize(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width, mode, positions):
    """(amplitude float32 (n, width), weight float32 (n), moment float32 (n, D), best int64 (n)).  x: the selected columns of file rows
    [x_row0, x_row0 + len(x)), any item type; [vb, ve): the recording; reference 0 / 1; ev_row any order."""
    wave = waveforms(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width)[0]
    return reduce_snippets(wave, ev_col0, positions32(positions, x.shape[1]), mode)


def location(moment, weight):
    """Step 6, the host's: float32(float64(moment) / float64(weight)), FILL where weight is 0 or the quotient is NaN."""
    moment, weight = np.asarray(moment, dtype=np.float32), np.asarray(weight, dtype=np.float32)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        loc = (moment.astype(np.float64) / weight.astype(np.float64)[:, None]).astype(np.float32)
    loc[np.isnan(loc) | (weight == 0)[:, None]] = FILL
    return loc


# ---- the same definition by brute force: every comparison and every step in plain loops, libm's fmaf --------------------------------
def reduce_brute(wave, col0, positions, mode):
    fmaf = _libm_fmaf()
    wave = np.asarray(wave, dtype=np.float32)
    n, T, W = wave.shape
    n_cols, D = positions.shape
    amp = np.full((n, W), FILL, np.float32)
    weight, moment, best = np.zeros(n, np.float32), np.zeros((n, D), np.float32), np.full(n, -1, np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for e in range(n):
            acc_w, acc_m, top = np.float32(0.0), [np.float32(0.0)] * D, None
            for w in range(W):
                lo = hi = ab = None
                for tau in range(T):
                    v = wave[e, tau, w]
                    if math.isnan(v):
                        continue
                    if lo is None or v < lo:
                        lo = v
                    if hi is None or v > hi:
                        hi = v
                    if ab is None or np.abs(v) > ab:
                        ab = np.abs(v)
                if lo is not None:
                    a = (hi - lo, -lo, hi, ab)[mode]
                    if not math.isnan(a):
                        amp[e, w] = a
                a = amp[e, w]
                if not math.isnan(a) and (top is None or a > top):
                    top, best[e] = a, w
                c = int(col0[e]) + w
                if not 0 <= c < n_cols:
                    continue
                g = a if a > 0 else np.float32(0.0)
                acc_w = np.float32(acc_w + g)
                acc_m = [fmaf(g, positions[c, d], acc_m[d]) for d in range(D)]
            weight[e] = FILL if math.isnan(acc_w) else acc_w
            for d in range(D):
                moment[e, d] = FILL if math.isnan(acc_m[d]) else acc_m[d]
    return amp, weight, moment, best


def localize_brute(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width, mode, positions):
    from tests.waveforms_oracle import waveforms_brute
    wave = waveforms_brute(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width)[0]
    return reduce_brute(wave, ev_col0, positions32(positions, x.shape[1]), mode)


class LocalizeOracleCodec(WaveformsOracleCodec):
    """WaveformsOracleCodec + localize restated in numpy, chunks read as waveforms reads them.  Records (lane, keys, lens, n_events) of
    every localize call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.localize_calls = []
        self.miss_next_localize = False              # simulate an entry dropped between the query and the call

    def localize(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols,
                 reference, ev_row, ev_col0, before, after, width, mode, positions, want_amp=True, lane=None):
        ev_row, ev_col0 = np.asarray(ev_row, dtype=np.int64), np.asarray(ev_col0, dtype=np.int64)
        self.localize_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(ev_row.size)))
        cols = np.asarray(cols, dtype=np.int64)
        taps = np.asarray(taps, dtype=np.float64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all() and reference in (0, 1) and mode in (0, 1, 2, 3)
        assert before >= 0 and after >= 0 and 1 <= before + after <= 4096 and 1 <= width <= 1024
        assert isinstance(positions, np.ndarray) and positions.dtype == np.float32 and positions.ndim == 2, 'positions'
        assert positions.shape[0] == cols.size and 1 <= positions.shape[1] <= MAX_DIMS and np.isfinite(positions).all(), 'positions'
        assert ev_row.size and (np.diff(ev_row) >= 0).all() and valid_begin <= ev_row[0] and ev_row[-1] < valid_end, 'events'
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        half = (taps.size - 1) // 2
        lo, hi = max(valid_begin, int(ev_row[0]) - before + half - (taps.size - 1)), min(valid_end, int(ev_row[-1]) + after + half)
        assert int(row0[0]) <= lo and hi <= int(row0[-1]) + int(n_rows[-1]), 'the chunks do not cover the rows read'
        status, arrays = self._call_chunks('localize', cache_id, keys, cdata, offs, lens, n_rows, n_channels, np.dtype(dtype), flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        amp, weight, moment, best = localize(x, int(row0[0]), valid_begin, valid_end, taps, reference, ev_row, ev_col0, before, after, width,
                                             mode, positions)
        return status, (amp if want_amp else None), weight, moment, best.astype(np.int32)
