"""Test-only restatements of mts_filtered_rank_hist in numpy, made of what the suite already trusts: z from tests/detect_oracle.py
(`filtered`, `row_median`) and the round from tests/select_oracle.py (`round_add`, `brute_round`) with z as a float32 "recording".  The
round is stated twice -- vectorised, and by a brute count per (window, column) cell with the median taken by sorting in Python -- and a
lane codec built on the first drives Reader.quantile / median / mad(taps=, reference=) on the CPU (argument handling, calls, lanes,
cache use, errors) and checks that every call's chunks are adjacent and cover its filter support."""
import math

import numpy as np

from mtscomp_amd import hip
from tests.detect_oracle import filtered, row_median
from tests.select_oracle import S, SelectOracleCodec, brute_round, empty_outputs, round_add


def z_rows(x, x_row0, vb, ve, a, b, taps, reference):
    """z[t] for file rows t in [a, b), float32: detect's.  x: the selected columns of file rows [x_row0, x_row0 + len(x))."""
    z = filtered(x, x_row0, vb, ve, a, b, np.asarray(taps, dtype=np.float64))
    if reference:
        with np.errstate(invalid='ignore', over='ignore'):
            z = (z - row_median(z)[:, None]).astype(np.float32)
    return z


def support(a, b, n_taps, vb, ve):
    """The file rows that z of rows [a, b) reads."""
    half = (n_taps - 1) // 2
    return max(vb, a + half - (n_taps - 1)), min(ve, b + half)


def filtered_round(x, x_row0, vb, ve, taps, reference, row_begin, row_end, window, count_begin, count_end, mode, center, pref, shift):
    """One round over the rows [count_begin, count_end) of the grid (row_begin, row_end, window) -> (hist, kmin, kmax, count)."""
    nw = -(-(row_end - row_begin) // window)
    out = empty_outputs(nw, x.shape[1])
    count = np.zeros(nw, np.int64)
    if count_end > count_begin:
        z = z_rows(x, x_row0, vb, ve, count_begin, count_end, taps, reference)
        count += round_add(out, z, count_begin, row_begin, row_end, window, mode, center, np.asarray(pref, np.uint64), np.asarray(shift, np.int64))
    return out + (count,)


def _sort_key(f):
    return (1, 0.0) if math.isnan(f) else (0, f)


def z_rows_brute(x, x_row0, vb, ve, a, b, taps, reference):
    """The same z with the median of every row taken by sorting its float32 values in Python."""
    z = filtered(x, x_row0, vb, ve, a, b, np.asarray(taps, dtype=np.float64))
    n = z.shape[1]
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
    return z


def filtered_round_brute(x, x_row0, vb, ve, taps, reference, row_begin, row_end, window, count_begin, count_end, mode, center, pref, shift):
    """The same round, cell by cell: the rows of window w inside the count range, one column at a time, counted in Python."""
    nw, C = -(-(row_end - row_begin) // window), x.shape[1]
    hist, kmin, kmax = empty_outputs(nw, C)
    count = np.zeros(nw, np.int64)
    for w in range(nw):
        a, b = max(count_begin, row_begin + w * window), min(count_end, row_end, row_begin + (w + 1) * window)
        if b <= a:
            continue
        count[w] = b - a
        z = z_rows_brute(x, x_row0, vb, ve, a, b, taps, reference)
        for j in range(C):
            h, mn, mx = brute_round(z[:, j], mode, None if center is None else float(center[w][j]), [int(p) for p in pref[w, :, j]],
                                    [int(s) for s in shift[w, :, j]])
            hist[w, :, :, j] = np.array(h, np.uint32)
            kmin[w, :, j] = np.array(mn, np.uint64)
            kmax[w, :, j] = np.array(mx, np.uint64)
    return hist, kmin, kmax, count


class FilteredSelectOracleCodec(SelectOracleCodec):
    """SelectOracleCodec + filtered_rank_hist restated in numpy: resident chunks read from the lane's cache dict (E_MISS when a chunk
    without bytes is not there), the others decoded and NOT inserted.  Records (lane, keys, lens, row_begin, row_end, count_begin,
    count_end, mode) of every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.filtered_calls = []
        self.miss_next_filtered_rank_hist = False    # simulate an entry dropped between the query and the call

    def filtered_rank_hist(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols,
                           reference, row_begin, row_end, window_rows, count_begin, count_end, mode, center, sel_prefix, sel_shift, lane=None):
        dtype = np.dtype(dtype)
        self.filtered_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(row_begin), int(row_end), int(count_begin),
                                    int(count_end), int(mode)))
        cols = np.asarray(cols, dtype=np.int64)
        taps = np.asarray(taps, dtype=np.float64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all()
        assert taps.ndim == 1 and 1 <= taps.size <= hip.DECIMATE_MAX_TAPS and np.isfinite(taps).all() and reference in (0, 1)
        assert not reference or cols.size <= hip.DETECT_MAX_REF_COLS
        assert valid_begin <= row_begin <= count_begin <= count_end <= row_end <= valid_end and window_rows >= 1
        nw = -(-(row_end - row_begin) // window_rows)
        pref, shift = np.asarray(sel_prefix, np.uint64), np.asarray(sel_shift, np.int64)
        assert pref.shape == (nw, S, cols.size) and shift.shape == pref.shape
        kb = hip.rank_key_bits(np.float32, mode)
        assert (shift <= kb - hip.RANK_BITS).all()
        assert all(int(p) >> (kb - int(s) - hip.RANK_BITS) == 0 for p, s in zip(pref[shift >= 0].ravel(), shift[shift >= 0].ravel()))
        assert mode in (0, 1, 2) and (not mode or np.asarray(center).shape == (nw, cols.size))
        # the chunks: adjacent, and they cover the filter's support of the count range
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        lo, hi = support(count_begin, count_end, taps.size, valid_begin, valid_end)
        assert count_end == count_begin or (int(row0[0]) <= lo and hi <= int(row0[-1]) + int(n_rows[-1])), 'support not covered'
        status, arrays = self._call_chunks('filtered_rank_hist', cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        hist, kmin, kmax, count = filtered_round(x, int(row0[0]), valid_begin, valid_end, taps, reference, row_begin, row_end, window_rows,
                                                 count_begin, count_end, mode, center, pref, shift)
        return status, dict(hist=hist, kmin=kmin, kmax=kmax, count=count)
