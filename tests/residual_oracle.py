"""Test-only restatements of mts_residual and mts_match_residual in numpy: the definition of include/mtscomp_hip.h twice -- vectorised
(on the filter and the median of tests/detect_oracle.py and the exact fmaf of tests/project_oracle.py, one fmaf of whole template rows
per (event, tau)) and by brute force (every entry its own scalar chain, with libm's fmaf where it can be loaded) -- and a lane codec
built on the first and on tests/tmatch_oracle.py so that the CPU suite drives Reader.residual and Reader.match_templates(subtract=)
(argument handling, calls, event slices, lanes, cache use, errors) and can check bit-identity."""
import numpy as np

from tests.correlate_oracle import FILL, _libm_fmaf, correlate_chain, reference_rows
from tests.project_oracle import fmaf_f32
from tests.tmatch_oracle import _NONE, TmatchOracleCodec, events_of_scores


def sort_events(sample, template, amplitude):
    """The list in the order of the definition: ascending sample, ties in list order.  -> (int64, int64, float32)."""
    sample = np.asarray(sample, np.int64).ravel()
    order = np.argsort(sample, kind='stable')
    with np.errstate(over='ignore'):
        return sample[order], np.asarray(template, np.int64).ravel()[order], np.asarray(amplitude).astype(np.float32).ravel()[order]


def _k32(templates):
    with np.errstate(over='ignore'):
        k = np.asarray(templates).astype(np.float32)
    return k[None] if k.ndim == 2 else k


def subtract_rows(z, z_row0, vb, ve, sample, template, amplitude, before, templates):
    """In place on z (float32, file rows [z_row0, z_row0 + len(z))): for the events in sorted order, every row of [vb, ve) that event e
    covers gets acc = fmaf(-amplitude[e], K[template[e], tau], acc).  Event after event is, row by row, the events that cover the row
    in list order; the rows outside [vb, ve) are not touched."""
    k = _k32(templates)
    T = k.shape[1]
    lo, hi = max(z_row0, vb), min(z_row0 + z.shape[0], ve)
    for s, o, a in zip(*sort_events(sample, template, amplitude)):
        t0, t1 = max(lo, s - before), min(hi, s - before + T)
        if t0 < t1:
            z[t0 - z_row0:t1 - z_row0] = fmaf_f32(-a, k[o, t0 - s + before:t1 - s + before], z[t0 - z_row0:t1 - z_row0])
    return z


def subtract_rows_t1(z, z_row0, vb, ve, sample, template, amplitude, before, templates):
    """subtract_rows for templates of one row (T = 1: an event covers the row sample - before alone), for lists too long to take event
    after event: the events of every rank within their row at once -- rank after rank is, row by row, list order."""
    k = _k32(templates)
    assert k.shape[1] == 1
    s, o, a = sort_events(sample, template, amplitude)
    t = s - before
    keep = (t >= max(z_row0, vb)) & (t < min(z_row0 + z.shape[0], ve))
    t, o, a = t[keep] - z_row0, o[keep], a[keep]
    first = np.r_[0, np.flatnonzero(np.diff(t)) + 1] if t.size else np.zeros(0, np.int64)
    rank = np.arange(t.size) - np.repeat(first, np.diff(np.r_[first, t.size]))
    for r in range(int(rank.max()) + 1 if t.size else 0):
        m = rank == r
        z[t[m]] = fmaf_f32(-a[m][:, None], k[o[m], 0], z[t[m]])
    return z


def residual(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates, sample, template, amplitude):
    """z' (i1 - i0, n_cols) float32 for file rows [i0, i1) of the recording [vb, ve).  x: the selected columns of file rows [x_row0,
    x_row0 + len(x)), any item type; reference 0 / 1; templates (K, T, n_cols), template row `before` on the event's sample.  A NaN
    has the bits 0x7fc00000."""
    assert vb <= i0 <= i1 <= ve
    z = subtract_rows(reference_rows(x, x_row0, vb, ve, i0, i1, taps, reference), i0, vb, ve, sample, template, amplitude, before, templates)
    z[np.isnan(z)] = FILL
    return z


def subtract_rows_brute(z, z_row0, vb, ve, sample, template, amplitude, before, templates):
    """subtract_rows by the words of the definition, into a new array: one scalar chain per (t, j) over the events that cover t, in
    list order."""
    fmaf = _libm_fmaf()
    k = _k32(templates)
    T = k.shape[1]
    ev = list(zip(*sort_events(sample, template, amplitude)))
    out = np.array(z, np.float32)
    for t in range(max(z_row0, vb), min(z_row0 + out.shape[0], ve)):
        mine = [(o, t - s + before, np.float32(-a)) for s, o, a in ev if 0 <= t - s + before < T]
        for j in range(out.shape[1]):
            acc = out[t - z_row0, j]
            for o, tau, na in mine:
                acc = fmaf(na, k[o, tau, j], acc)
            out[t - z_row0, j] = acc
    return out


def residual_brute(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates, sample, template, amplitude):
    z = subtract_rows_brute(reference_rows(x, x_row0, vb, ve, i0, i1, taps, reference), i0, vb, ve, sample, template, amplitude, before, templates)
    z[np.isnan(z)] = FILL
    return z


def residual_scores(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates, sample, template, amplitude):
    """correlate's chain on z' for file rows [i0, i1): z' inside the recording, +0 outside it."""
    T = _k32(templates).shape[1]
    a = i0 - before
    z = reference_rows(x, x_row0, vb, ve, a, i1 - before + T - 1, taps, reference)
    return correlate_chain(subtract_rows(z, a, vb, ve, sample, template, amplitude, before, templates), templates)


def match_residual(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates, threshold, R, sample, template, amplitude):
    """(row int64, template int64, score float32) of the events of rows [i0, i1) of the scores of z' (tests/tmatch_oracle.py)."""
    if i1 <= i0:
        return _NONE
    a, b = max(vb, i0 - R), min(ve, i1 + R)
    score = residual_scores(x, x_row0, vb, ve, a, b, taps, reference, before, templates, sample, template, amplitude)
    return events_of_scores(score, a, i0, i1, threshold, R)


class ResidualOracleCodec(TmatchOracleCodec):
    """TmatchOracleCodec + residual and match_residual restated in numpy.  Records (lane, keys, lens, row_begin, row_end, the event
    rows) of every residual call and (lane, keys, lens, row_begin, row_end, max_events, the event rows) of every match_residual
    call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.residual_calls = []
        self.match_residual_calls = []
        self.miss_next_residual = False
        self.miss_next_match_residual = False

    @staticmethod
    def _check_events(sub_row, sub_tpl, sub_amp, vb, ve, n_out):
        row, tpl, amp = np.asarray(sub_row), np.asarray(sub_tpl), np.asarray(sub_amp)
        assert (row.dtype, tpl.dtype, amp.dtype) == (np.int64, np.int32, np.float32) and row.ndim == 1 and row.shape == tpl.shape == amp.shape
        assert (np.diff(row) >= 0).all() and ((row >= vb) & (row < ve)).all() and ((tpl >= 0) & (tpl < n_out)).all() and np.isfinite(amp).all()
        return row, tpl, amp

    def residual(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end,
                 taps, cols, reference, before, templates, sub_row, sub_tpl, sub_amp, lane=None):
        cols = np.asarray(cols, dtype=np.int64)
        taps = np.asarray(taps, dtype=np.float64)
        k = np.asarray(templates)
        assert 1 <= cols.size <= 1024 and (cols >= 0).all() and (cols < n_channels).all() and reference in (0, 1)
        assert k.ndim == 3 and k.dtype == np.float32 and k.shape[2] == cols.size and 1 <= k.shape[0] <= 1024 and 1 <= k.shape[1] <= 256
        assert np.isfinite(k).all() and 0 <= before <= k.shape[1]
        assert valid_begin <= row_begin < row_end <= valid_end
        ev = self._check_events(sub_row, sub_tpl, sub_amp, valid_begin, valid_end, k.shape[0])
        self.residual_calls.append((lane, [int(v) for v in keys], [int(n) for n in lens], int(row_begin), int(row_end), ev[0].tolist()))
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        half = (taps.size - 1) // 2
        lo, hi = max(valid_begin, row_begin + half - (taps.size - 1)), min(valid_end, row_end + half)
        assert lo < hi and int(row0[0]) <= lo and hi <= int(row0[-1]) + int(n_rows[-1]), 'the chunks do not cover the rows read'
        status, arrays = self._call_chunks('residual', cache_id, keys, cdata, offs, lens, n_rows, n_channels, np.dtype(dtype), flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        return status, residual(x, int(row0[0]), valid_begin, valid_end, row_begin, row_end, taps, reference, before, k, *ev)

    def match_residual(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin,
                       row_end, taps, cols, reference, before, templates, threshold, exclude_rows, max_events, sub_row, sub_tpl, sub_amp,
                       lane=None):
        cols = np.asarray(cols, dtype=np.int64)
        taps = np.asarray(taps, dtype=np.float64)
        k = np.asarray(templates)
        thr = np.asarray(threshold)
        assert 1 <= cols.size <= 1024 and (cols >= 0).all() and (cols < n_channels).all() and reference in (0, 1)
        assert k.ndim == 3 and k.dtype == np.float32 and k.shape[2] == cols.size and 1 <= k.shape[0] <= 1024 and 1 <= k.shape[1] <= 256
        assert np.isfinite(k).all() and 0 <= before <= k.shape[1]
        assert thr.dtype == np.float32 and thr.shape == (k.shape[0],) and np.isfinite(thr).all()
        assert 0 <= exclude_rows <= 255 and max_events >= 0
        assert valid_begin <= row_begin < row_end <= valid_end
        ev = self._check_events(sub_row, sub_tpl, sub_amp, valid_begin, valid_end, k.shape[0])
        self.match_residual_calls.append((lane, [int(v) for v in keys], [int(n) for n in lens], int(row_begin), int(row_end), int(max_events),
                                          ev[0].tolist()))
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        half = (taps.size - 1) // 2
        lo = max(valid_begin, row_begin - exclude_rows - before + half - (taps.size - 1))
        hi = min(valid_end, row_end + exclude_rows + k.shape[1] - before - 1 + half)
        if lo < hi:
            assert len(keys) and int(row0[0]) <= lo and hi <= int(row0[-1]) + int(n_rows[-1]), 'the chunks do not cover the rows read'
        else:
            assert not len(keys), 'chunks for rows that read nothing'
        status, arrays = self._call_chunks('match_residual', cache_id, keys, cdata, offs, lens, n_rows, n_channels, np.dtype(dtype), flags,
                                           fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols] if arrays else np.zeros((0, cols.size), np.dtype(dtype))
        row, tpl, val = match_residual(x, int(row0[0]) if len(keys) else 0, valid_begin, valid_end, row_begin, row_end, taps, reference, before,
                                       k, thr, exclude_rows, *ev)
        n = min(row.size, int(max_events))
        return status, int(row.size), row[:n], tpl[:n].astype(np.int32), val[:n]
