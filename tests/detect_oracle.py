"""Test-only restatements of mts_detect in numpy: the definition of include/mtscomp_hip.h twice -- vectorised (built on
fir_decimate, np.sort for the median, shifted comparisons at the candidates) and by brute force (plain loops over every sample
and neighbour) -- and a lane codec built on the first so that the CPU suite drives Reader.detect (argument handling, calls,
lanes, cache use, the second call of a short buffer, errors) and can check bit-identity."""
import math

import numpy as np

from tests.codec_oracle import LaneOracleCodec
from tests.decimate_oracle import fir_decimate

SIGNS = {'neg': 0, 'pos': 1, 'both': 2}


def _value(z, sign):
    return -z if sign == 0 else z if sign == 1 else np.abs(z)


def filtered(x, x_row0, vb, ve, a, b, taps):
    """y[t] for file rows t in [a, b): the float32 FIR of decimate(1, edge='recording') (newest row t + half)."""
    half = (len(taps) - 1) // 2
    return fir_decimate(x, x_row0, vb, ve, a + half, b - a, 1, taps, np.float32)


def row_median(y):
    """float32 median of every row: np.sort's order (NaN last), 0.5f * (a + b) for an even n, NaN when the row holds one."""
    n = y.shape[1]
    ys = np.sort(y, axis=1)
    with np.errstate(invalid='ignore', over='ignore'):
        m = ys[:, (n - 1) // 2] if n % 2 else np.float32(0.5) * (ys[:, n // 2 - 1] + ys[:, n // 2])
    m = m.astype(np.float32)
    m[np.isnan(ys[:, -1])] = np.nan
    return m


def detect_events(x, x_row0, vb, ve, i0, i1, taps, threshold, sign, reference, R, S):
    """(row int64, pos int64, amp float32) of the events of rows [i0, i1) in (row, pos) order.  x: the selected columns of file
    rows [x_row0, x_row0 + len(x)), any item type; [vb, ve): the recording; sign 0 / 1 / 2; reference 0 / 1."""
    n = x.shape[1]
    taps = np.asarray(taps, dtype=np.float64)
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float32), (n,))
    a, b = max(vb, i0 - R), min(ve, i1 + R)
    if i1 <= i0 or not n:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    z = filtered(x, x_row0, vb, ve, a, b, taps)
    if reference:
        with np.errstate(invalid='ignore', over='ignore'):
            z = (z - row_median(z)[:, None]).astype(np.float32)
    return events_of(z, a, i0, i1, thr, sign, R, S)


def events_of(z, a, i0, i1, thr, sign, R, S):
    """The events of file rows [i0, i1) given z (float32) for file rows [a, a + len(z)): every row of the recording within R of them."""
    n = z.shape[1]
    v = _value(z, sign)
    with np.errstate(invalid='ignore'):
        cand = v > thr[None, :]
    cand[:i0 - a] = False
    cand[i1 - a:] = False
    ti, ji = np.nonzero(cand)                                    # row-major: the (t, j) order
    # the candidates still alive against one offset after the other, nearest first (the order decides nothing but the time)
    for dt, dj in sorted(((dt, dj) for dt in range(-R, R + 1) for dj in range(-S, S + 1) if dt or dj), key=lambda o: (abs(o[0]), abs(o[1]))):
        if not ti.size:
            break
        t2, j2 = ti + dt, ji + dj
        ok = (t2 >= 0) & (t2 < v.shape[0]) & (j2 >= 0) & (j2 < n)
        vc = v[ti, ji]
        vn = np.full(ti.size, np.nan, np.float32)
        vn[ok] = v[t2[ok], j2[ok]]
        with np.errstate(invalid='ignore'):
            beat = vn > vc
            if dt < 0 or (dt == 0 and dj < 0):
                beat |= vn == vc
        ti, ji = ti[~beat], ji[~beat]
    return (ti + a).astype(np.int64), ji.astype(np.int64), z[ti, ji].astype(np.float32)


def tied_events(x, x_row0, vb, ve, i0, i1, taps, sign, reference, R, S, row, pos):
    """How many of the events (row, pos) have a neighbour of exactly their detection value."""
    a, b = max(vb, i0 - R), min(ve, i1 + R)
    z = filtered(x, x_row0, vb, ve, a, b, np.asarray(taps, dtype=np.float64))
    if reference:
        z = (z - row_median(z)[:, None]).astype(np.float32)
    v = _value(z, sign)
    n_tied = 0
    for t, j in zip(row - a, pos):
        t0, t1, j0, j1 = max(0, t - R), min(v.shape[0], t + R + 1), max(0, j - S), min(v.shape[1], j + S + 1)
        n_tied += int((v[t0:t1, j0:j1] == v[t, j]).sum() > 1)
    return n_tied


# ---- the same definition by brute force: no numpy in the median, the comparisons or the order -------------------------------------
def _sort_key(f):
    return (1, 0.0) if math.isnan(f) else (0, f)


def detect_events_brute(x, x_row0, vb, ve, i0, i1, taps, threshold, sign, reference, R, S):
    n = x.shape[1]
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float32), (n,))
    a, b = max(vb, i0 - R), min(ve, i1 + R)
    if i1 <= i0 or not n:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    z = filtered(x, x_row0, vb, ve, a, b, np.asarray(taps, dtype=np.float64))
    if reference:
        for t in range(z.shape[0]):
            vals = sorted((np.float32(f) for f in z[t]), key=_sort_key)
            with np.errstate(invalid='ignore', over='ignore'):
                if any(math.isnan(f) for f in vals):
                    m = np.float32(np.nan)
                elif n % 2:
                    m = vals[(n - 1) // 2]
                else:
                    m = np.float32(0.5) * np.float32(vals[n // 2 - 1] + vals[n // 2])
                z[t] = z[t] - m
    v = _value(z, sign)
    rows, poss, amps = [], [], []
    for t in range(i0, i1):
        for j in range(n):
            mine = v[t - a, j]
            if not mine > thr[j]:
                continue
            beaten = False
            for t2 in range(max(a, t - R), min(b, t + R + 1)):
                for j2 in range(max(0, j - S), min(n, j + S + 1)):
                    if (t2, j2) == (t, j):
                        continue
                    other = v[t2 - a, j2]
                    if other > mine or (other == mine and (t2, j2) < (t, j)):
                        beaten = True
                        break
                if beaten:
                    break
            if not beaten:
                rows.append(t)
                poss.append(j)
                amps.append(z[t - a, j])
    return np.array(rows, np.int64), np.array(poss, np.int64), np.array(amps, np.float32)


class DetectOracleCodec(LaneOracleCodec):
    """LaneOracleCodec + detect restated in numpy: resident chunks read from the lane's cache dict (E_MISS when a chunk without
    bytes is not there), the others decoded and NOT inserted.  Records (lane, keys, lens, max_events) of every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.detect_calls = []
        self.miss_next_detect = False                # simulate an entry dropped between the query and the call

    def detect(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end,
               taps, cols, threshold, sign, reference, exclude_rows, exclude_cols, max_events, lane=None):
        dtype = np.dtype(dtype)
        self.detect_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(max_events)))
        cols = np.asarray(cols, dtype=np.int64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all()
        assert sign in (0, 1, 2) and reference in (0, 1) and max_events >= 0
        assert valid_begin <= row_begin <= row_end <= valid_end
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        status, arrays = self._call_chunks('detect', cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        row, pos, amp = detect_events(x, int(row0[0]), valid_begin, valid_end, row_begin, row_end, taps, threshold, sign, reference,
                                      exclude_rows, exclude_cols)
        k = min(row.size, int(max_events))
        return status, int(row.size), row[:k], pos[:k].astype(np.int32), amp[:k]
