"""Test-only restatements of mts_filtered_gram in numpy, made of what the suite already trusts: z from tests/filtered_select_oracle.py
(`z_rows`, detect's z) and the partials from tests/gram_oracle.py (`gram_partials`) with z as a float32 "recording".  The partials are
stated twice -- through those two, and by a brute form: z with every row's median taken by sorting in Python (`z_rows_brute`) and a
plain per-group Gram in np.longdouble -- and a lane codec built on the first drives Reader.cov(taps=, reference=) on the CPU (argument
handling, calls, lanes, cache use, errors) and checks that every call's chunks are adjacent and cover its filter support."""
import numpy as np

from mtscomp_amd import hip
from tests.filtered_select_oracle import support, z_rows, z_rows_brute
from tests.gram_oracle import GramOracleCodec, gram_partials


def call_rows(range_begin, range_end, window_rows, group_begin, group_end):
    """The file rows [lo, hi) of groups [group_begin, group_end) of the grid (adjacent: one run of rows)."""
    return (hip.gram_group_rows(range_begin, range_end, window_rows, group_begin)[0],
            hip.gram_group_rows(range_begin, range_end, window_rows, group_end - 1)[1])


def filtered_partials(x, x_row0, vb, ve, taps, reference, range_begin, range_end, window_rows, group_begin, group_end):
    """The partials mts_filtered_gram returns: gram_partials of z of the call's rows.  x: the selected columns of file rows
    [x_row0, x_row0 + len(x)).  -> (gram (n, C, C) float64, sum (n, C) float64)."""
    lo, hi = call_rows(range_begin, range_end, window_rows, group_begin, group_end)
    z = z_rows(x, x_row0, vb, ve, lo, hi, taps, reference)
    assert z.dtype == np.float32
    return gram_partials(z, lo, range_begin, range_end, window_rows, group_begin, group_end)


def filtered_partials_brute(x, x_row0, vb, ve, taps, reference, range_begin, range_end, window_rows, group_begin, group_end):
    """The same partials, group by group: z of the group's rows with the median of every row taken by sorting in Python, then
    sum_t z[t, i] z[t, j] and sum_t z[t, i] in np.longdouble.  -> (gram (n, C, C) longdouble, sum (n, C) longdouble, absgram (n, C, C)
    float64: sum_t |z[t, i] z[t, j]|, what gram_bound is taken from, rows (n,): the rows of each group)."""
    n, C = group_end - group_begin, x.shape[1]
    G, S, A, rows = np.zeros((n, C, C), np.longdouble), np.zeros((n, C), np.longdouble), np.zeros((n, C, C)), np.zeros(n, np.int64)
    for j in range(n):
        lo, hi = hip.gram_group_rows(range_begin, range_end, window_rows, group_begin + j)
        z = z_rows_brute(x, x_row0, vb, ve, lo, hi, taps, reference).astype(np.float64)
        zl = z.astype(np.longdouble)
        with np.errstate(invalid='ignore', over='ignore'):
            for t in range(z.shape[0]):
                G[j] += np.outer(zl[t], zl[t])
                S[j] += zl[t]
                A[j] += np.outer(np.abs(z[t]), np.abs(z[t]))
        rows[j] = hi - lo
    return G, S, A, rows


class FilteredGramOracleCodec(GramOracleCodec):
    """GramOracleCodec + filtered_gram restated in numpy: resident chunks read from the lane's cache dict (E_MISS when a chunk without
    bytes is not there), the others decoded and NOT inserted.  Records (lane, keys, lens, range_begin, range_end, window_rows,
    group_begin, group_end) of every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.filtered_gram_calls = []
        self.miss_next_filtered_gram = False         # simulate an entry dropped between the query and the call

    def filtered_gram(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference,
                      range_begin, range_end, window_rows, group_begin, group_end, lane=None):
        dtype = np.dtype(dtype)
        self.filtered_gram_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(range_begin), int(range_end), int(window_rows),
                                         int(group_begin), int(group_end)))
        cols = np.asarray(cols, dtype=np.int64)
        taps = np.asarray(taps, dtype=np.float64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all()
        assert taps.ndim == 1 and 1 <= taps.size <= hip.DECIMATE_MAX_TAPS and np.isfinite(taps).all() and reference in (0, 1)
        assert cols.size <= (hip.DETECT_MAX_REF_COLS if reference else hip.GRAM_MAX_COLS)
        assert valid_begin <= range_begin < range_end <= valid_end and window_rows >= 1
        assert 0 <= group_begin < group_end <= hip.gram_groups(range_begin, range_end, window_rows)
        # the chunks: adjacent, and they cover the filter's support of the call's groups
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        lo, hi = support(*call_rows(range_begin, range_end, window_rows, group_begin, group_end), taps.size, valid_begin, valid_end)
        assert int(row0[0]) <= lo and hi <= int(row0[-1]) + int(n_rows[-1]), 'support not covered'
        status, arrays = self._call_chunks('filtered_gram', cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        G, S = filtered_partials(x, int(row0[0]), valid_begin, valid_end, taps, reference, range_begin, range_end, window_rows, group_begin,
                                 group_end)
        return status, G, S
