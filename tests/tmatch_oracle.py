"""Test-only restatements of mts_match_templates in numpy: the definition of include/mtscomp_hip.h twice over the scores of
tests/correlate_oracle.correlate -- vectorised through the row maximum (the equivalent form the kernels use) and as the plain loop
over every (t', k') -- and a lane codec built on the first so that the CPU suite drives Reader.match_templates (argument handling,
calls, lanes, cache use, the second call of a short buffer, errors) and can check bit-identity."""
import numpy as np

from tests.codec_oracle import LaneOracleCodec
from tests.correlate_oracle import correlate

_NONE = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))


def events_of_scores(score, a, i0, i1, threshold, R):
    """The events of file rows [i0, i1) given score (float32, rows x K) of file rows [a, a + len(score)): every row of the recording
    within R of them.  Through the row maximum: b[t] the largest score that is not a NaN, k*[t] the first template that attains it; an
    event when b > threshold[k*], no earlier row within R has b >= b[t] and no later one b > b[t].  -> (row, template, score)."""
    score = np.asarray(score, np.float32)
    n, n_out = score.shape
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float32), (n_out,))
    if i1 <= i0:
        return _NONE
    nan = np.isnan(score)
    none = nan.all(axis=1)
    best = np.where(nan, -np.inf, score).max(axis=1).astype(np.float32)          # (-0 == +0: the comparisons below do not care which)
    arg = (np.where(nan, -np.inf, score) == best[:, None]).argmax(axis=1)       # the first template that attains it
    arg[none] = 0
    b = np.where(none, np.float32(np.nan), best).astype(np.float32)             # a row of NaNs beats nothing: its NaN compares false
    with np.errstate(invalid='ignore'):
        alive = b > thr[arg]
    alive[:i0 - a] = False
    alive[i1 - a:] = False
    ti = np.nonzero(alive)[0]
    for d in range(1, R + 1):
        for dt in (-d, d):
            if not ti.size:
                break
            t2 = ti + dt
            ok = (t2 >= 0) & (t2 < n)
            vn = np.full(ti.size, np.nan, np.float32)
            vn[ok] = b[t2[ok]]
            with np.errstate(invalid='ignore'):
                beat = (vn >= b[ti]) if dt < 0 else (vn > b[ti])
            ti = ti[~beat]
    return (ti + a).astype(np.int64), arg[ti].astype(np.int64), score[ti, arg[ti]].astype(np.float32)


def events_of_scores_brute(score, a, i0, i1, threshold, R):
    """The same events by the words of the definition: (t, k) with score > threshold[k] that no (t', k') within R rows beats --
    score' > score, or equal at an earlier (row, template)."""
    score = np.asarray(score, np.float32)
    n, n_out = score.shape
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float32), (n_out,))
    rows, tpls, vals = [], [], []
    for t in range(i0, i1):
        for k in range(n_out):
            mine = score[t - a, k]
            if not mine > thr[k]:
                continue
            beaten = False
            for t2 in range(max(a, t - R), min(a + n, t + R + 1)):
                for k2 in range(n_out):
                    other = score[t2 - a, k2]
                    if other > mine or (other == mine and (t2, k2) < (t, k)):
                        beaten = True
                        break
                if beaten:
                    break
            if not beaten:
                rows.append(t)
                tpls.append(k)
                vals.append(mine)
    return np.array(rows, np.int64), np.array(tpls, np.int64), np.array(vals, np.float32)


def _scores(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates, R):
    a, b = max(vb, i0 - R), min(ve, i1 + R)
    return a, correlate(x, x_row0, vb, ve, a, b, taps, reference, before, templates)


def match_templates(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates, threshold, R):
    """(row int64, template int64, score float32) of the events of rows [i0, i1), ascending.  x: the selected columns of file rows
    [x_row0, x_row0 + len(x)), any item type (no rows at all when the events read none); [vb, ve): the recording; reference 0 / 1;
    templates (K, T, n_cols), template row `before` on the scored row; threshold a number or one per template."""
    if i1 <= i0:
        return _NONE
    a, score = _scores(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates, R)
    return events_of_scores(score, a, i0, i1, threshold, R)


def match_templates_brute(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates, threshold, R):
    if i1 <= i0:
        return _NONE
    a, score = _scores(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates, R)
    return events_of_scores_brute(score, a, i0, i1, threshold, R)


class TmatchOracleCodec(LaneOracleCodec):
    """LaneOracleCodec + match_templates restated in numpy: resident chunks read from the lane's cache dict (E_MISS when a chunk
    without bytes is not there), the others decoded and NOT inserted.  Records (lane, keys, lens, row_begin, row_end, max_events) of
    every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.match_templates_calls = []
        self.miss_next_match_templates = False       # simulate an entry dropped between the query and the call

    def match_templates(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin,
                        row_end, taps, cols, reference, before, templates, threshold, exclude_rows, max_events, lane=None):
        self.match_templates_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(row_begin), int(row_end), int(max_events)))
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
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        half = (taps.size - 1) // 2
        lo = max(valid_begin, row_begin - exclude_rows - before + half - (taps.size - 1))
        hi = min(valid_end, row_end + exclude_rows + k.shape[1] - before - 1 + half)
        if lo < hi:
            assert len(keys) and int(row0[0]) <= lo and hi <= int(row0[-1]) + int(n_rows[-1]), 'the chunks do not cover the rows read'
        else:
            assert not len(keys), 'chunks for rows that read nothing'
        status, arrays = self._call_chunks('match_templates', cache_id, keys, cdata, offs, lens, n_rows, n_channels, np.dtype(dtype), flags,
                                           fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols] if arrays else np.zeros((0, cols.size), np.dtype(dtype))
        row, tpl, val = match_templates(x, int(row0[0]) if len(keys) else 0, valid_begin, valid_end, row_begin, row_end, taps, reference, before,
                                        k, thr, exclude_rows)
        n = min(row.size, int(max_events))
        return status, int(row.size), row[:n], tpl[:n].astype(np.int32), val[:n]
