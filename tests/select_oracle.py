"""Test-only restatements of mts_rank_hist in numpy: the order keys, one round of the radix select (digit histograms, kmin / kmax of a
selector's candidates), a lane codec built on it so that the CPU suite drives Reader.quantile / median / mad (argument handling, rounds,
calls, lanes, cache use, errors), and the references the results are held to: np.sort for the order statistics, np.median, np.quantile
and scipy.stats.median_abs_deviation."""
from fractions import Fraction

import numpy as np

from mtscomp_amd import hip
from tests.codec_oracle import LaneOracleCodec

S, BITS = hip.RANK_SELECTORS, hip.RANK_BITS
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys_of(x, mode=0, center=None):
    """The order keys, stated without hip.rank_keys: floats through their bit patterns, integers through an offset."""
    x = np.asarray(x)
    if mode:
        with np.errstate(invalid='ignore', over='ignore'):
            x = x.astype(np.float64) - (0.0 if center is None else center)
        x = np.abs(x) if mode == 2 else x
    if x.dtype.kind == 'f':
        nb = 8 * x.dtype.itemsize
        out = np.empty(x.shape, np.uint64)
        flat, o = x.ravel(), out.ravel()
        ints = np.ascontiguousarray(flat).view('u%d' % x.dtype.itemsize)
        for i in range(flat.size):
            b = int(ints[i])
            if flat[i] != flat[i]:
                o[i] = (1 << nb) - 1
            elif flat[i] == 0:
                o[i] = 1 << (nb - 1)
            else:
                o[i] = ((1 << nb) - 1 - b) if b >> (nb - 1) else b + (1 << (nb - 1))
        return out
    if x.dtype.kind == 'u':
        return x.astype(np.uint64)
    return (x.astype(object) + (1 << (8 * x.dtype.itemsize - 1))).astype(np.uint64)


def empty_outputs(n_windows, n_cols):
    return (np.zeros((n_windows, S, 1 << BITS, n_cols), np.uint32), np.full((n_windows, S, n_cols), ONES, np.uint64),
            np.zeros((n_windows, S, n_cols), np.uint64))


def round_add(out, x, x_row0, row_begin, row_end, window, mode, center, pref, shift):
    """Adds one chunk's items x (rows, C: the columns already chosen; file rows from x_row0) to the outputs `out` = (hist, kmin, kmax)
    of a round on the grid (row_begin, row_end, window).  -> rows counted per window."""
    hist, kmin, kmax = out
    nw, C = pref.shape[0], pref.shape[2]
    lo, hi = max(row_begin, x_row0), min(row_end, x_row0 + x.shape[0])
    count = np.zeros(nw, np.int64)
    if hi <= lo or not C:
        return count
    rows = np.arange(lo, hi)
    w = (rows - row_begin) // window
    np.add.at(count, w, 1)
    cen = None if center is None else np.asarray(center, np.float64)[w]
    k = hip.rank_keys(x[lo - x_row0:hi - x_row0], mode, cen)
    ww = np.repeat(w[:, None], C, axis=1)
    jj = np.repeat(np.arange(C)[None, :], len(rows), axis=0)
    for s in range(S):
        sh = shift[w, s].astype(np.int64)                         # (rows, C)
        act = sh >= 0
        shu = np.where(act, sh, 0).astype(np.uint64)
        whole = shu + np.uint64(BITS) >= np.uint64(64)
        top = np.where(whole, np.uint64(0), k >> np.where(whole, np.uint64(0), shu + np.uint64(BITS)))
        cand = act & (top == pref[w, s])
        dig = ((k >> shu) & np.uint64((1 << BITS) - 1)).astype(np.int64)
        np.add.at(hist, (ww[cand], s, dig[cand], jj[cand]), 1)
        np.minimum.at(kmin, (ww[cand], s, jj[cand]), k[cand])
        np.maximum.at(kmax, (ww[cand], s, jj[cand]), k[cand])
    return count


def brute_round(x, mode, center, pref, shift):
    """One window, one column, by counting in Python: (hist[S][256], kmin[S], kmax[S]) of the items x (1-D)."""
    ks = [int(v) for v in keys_of(x, mode, center)]
    hist = [[0] * (1 << BITS) for _ in range(S)]
    kmin, kmax = [int(ONES)] * S, [0] * S
    for s in range(S):
        if shift[s] < 0:
            continue
        for k in ks:
            if k >> (shift[s] + BITS) == pref[s]:
                hist[s][(k >> shift[s]) & 255] += 1
                kmin[s], kmax[s] = min(kmin[s], k), max(kmax[s], k)
    return hist, kmin, kmax


class SelectOracleCodec(LaneOracleCodec):
    """LaneOracleCodec + rank_hist restated in numpy: resident chunks read from the lane's cache dict (E_MISS when a chunk without bytes
    is not there), the others decoded and NOT inserted.  Records (lane, keys, lens, row_begin, row_end, mode) of every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.rank_calls = []

    def rank_hist(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, row_begin, row_end, window_rows, cols, mode,
                  center, sel_prefix, sel_shift, lane=None):
        dtype = np.dtype(dtype)
        self.rank_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(row_begin), int(row_end), int(mode)))
        cols = np.asarray(cols, dtype=np.int64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all()
        nw = -(-(row_end - row_begin) // window_rows)
        pref, shift = np.asarray(sel_prefix, np.uint64), np.asarray(sel_shift, np.int64)
        assert pref.shape == (nw, S, cols.size) and shift.shape == pref.shape
        kb = hip.rank_key_bits(dtype, mode)
        assert (shift <= kb - BITS).all()
        assert all(int(p) >> (kb - int(s) - BITS) == 0 for p, s in zip(pref[shift >= 0].ravel(), shift[shift >= 0].ravel()))
        assert mode in (0, 1, 2) and (not mode or np.asarray(center).shape == (nw, cols.size))
        out = empty_outputs(nw, cols.size)
        count = np.zeros(nw, np.int64)
        status, arrays = self._call_chunks('rank_hist', cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags)
        for r0, st, a in zip(row0, status, arrays):
            if st == 0:
                count += round_add(out, a[:, cols], int(r0), row_begin, row_end, window_rows, mode, center, pref, shift)
        return status, dict(hist=out[0], kmin=out[1], kmax=out[2], count=count)


# ---- the references ------------------------------------------------------------------------------------------------------------------
def ordered(x, mode=0, center=None):
    """What is ordered, sorted along axis 0 by numpy: the items (mode 0) or the float64 differences / their absolute values."""
    x = np.asarray(x)
    if mode:
        with np.errstate(invalid='ignore', over='ignore'):
            x = x.astype(np.float64) - (0.0 if center is None else center)
        x = np.abs(x) if mode == 2 else x
    return np.sort(x, axis=0)


def position(q, n):
    """(index, frac, upper index) of quantile q in n rows, with the position q * (n - 1) computed exactly."""
    v = Fraction(float(q)) * (n - 1)
    j = v.numerator // v.denominator
    return j, float(v - j), min(j + 1, n - 1)


def same_values(a, b):
    """Equal by value (NaN equals NaN, -0 equals +0); integers also by dtype and bytes."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind in 'iu':
        return a.tobytes() == np.ascontiguousarray(b).tobytes()
    return bool(np.array_equal(a, b, equal_nan=True))


def windows_of(n, start, stop, window):
    window = window or max(stop - start, 1)
    return [(a, min(a + window, stop)) for a in range(start, stop, window)]


def check_quantile(got, x, start, stop, window, q, method, mode=0, center=None):
    """A Reader.quantile result (arrays (n_windows, n_q, C)) against the items x (columns chosen): count, index, frac, lower / upper
    against the sorted items, and the value formed as the interface states it."""
    wins = windows_of(x.shape[0], start, stop, window)
    q = np.atleast_1d(np.asarray(q, np.float64))
    assert got.count.tolist() == [b - a for a, b in wins]
    assert got.quantile.shape == (len(wins), q.size, x.shape[1]) and got.quantile.dtype == np.float64
    assert got.lower.dtype == (np.float64 if mode else x.dtype) and got.upper.dtype == got.lower.dtype
    for w, (a, b) in enumerate(wins):
        cen = None if center is None else np.broadcast_to(center, (len(wins), x.shape[1]))[w]
        srt = ordered(x[a:b], mode, cen)
        nan = np.isnan(srt).any(axis=0) if srt.dtype.kind == 'f' else np.zeros(x.shape[1], bool)
        for k, qv in enumerate(q):
            j, g, j1 = position(qv, b - a)
            assert (got.index[w, k], got.frac[w, k]) == (j, g)
            assert same_values(got.lower[w, k], srt[j]) and same_values(got.upper[w, k], srt[j1]), (w, k)
            lo, hi = srt[j].astype(np.float64), srt[j1].astype(np.float64)
            with np.errstate(invalid='ignore', over='ignore'):
                want = {'linear': lo + (hi - lo) * g, 'lower': lo, 'higher': hi if g > 0 else lo,
                        'midpoint': (lo + hi) / 2 if g > 0 else lo,
                        'nearest': lo if g < 0.5 else hi if g > 0.5 else (lo if j % 2 == 0 else hi)}[method]
            want = np.where(nan, np.nan, want)
            assert same_values(got.quantile[w, k], want), (w, k, method)


def np_median(x, start, stop, window):
    with np.errstate(invalid='ignore', over='ignore'):
        rows = [np.median(x[a:b].astype(np.float64), axis=0) for a, b in windows_of(x.shape[0], start, stop, window)]
    return np.array(rows, np.float64).reshape(len(rows), x.shape[1])


def scipy_mad(x, start, stop, window, center=None):
    """scipy.stats.median_abs_deviation per window; with a center (it broadcasts to (n_windows, C)) np.median(|x - center|)."""
    from scipy.stats import median_abs_deviation
    wins = windows_of(x.shape[0], start, stop, window)
    cen = None if center is None else np.broadcast_to(np.asarray(center, np.float64), (len(wins), x.shape[1]))
    rows = []
    for w, (a, b) in enumerate(wins):
        xf = x[a:b].astype(np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            rows.append(median_abs_deviation(xf, axis=0) if cen is None else np.median(np.abs(xf - cen[w]), axis=0))
    return np.array(rows, np.float64).reshape(len(rows), x.shape[1])


def walk_select(round_fn, n_windows, n_cols, ranks, key_bits):
    """A plain most-significant-digit walk (no bits skipped) for two ranks per window, driving `round_fn(prefix, shift) -> dict
    hist / kmin / kmax` directly: what a caller of the C ABI would write.  ranks: (n_windows, 2).  The two ranks of a cell share
    selector 0 while their prefixes agree.  -> keys (n_windows, 2, n_cols) uint64."""
    pref = np.zeros((n_windows, S, n_cols), np.uint64)
    rel = np.repeat(np.asarray(ranks, np.int64)[:, :, None], n_cols, axis=2)
    for shift in range(key_bits - BITS, -1, -BITS):
        share = pref[:, 0] == pref[:, 1]
        sel_shift = np.full((n_windows, S, n_cols), shift, np.int32)
        sel_shift[:, 1][share] = -1
        res = round_fn(pref, sel_shift)
        for s in range(S):
            h = np.where(share[:, None, :], res['hist'][:, 0], res['hist'][:, s]).astype(np.int64) if s else res['hist'][:, 0].astype(np.int64)
            cum = np.cumsum(h, axis=1)
            assert (rel[:, s] < cum[:, -1]).all()
            dig = (cum <= rel[:, s][:, None, :]).sum(axis=1)
            rel[:, s] -= np.take_along_axis(cum - h, dig[:, None, :], axis=1)[:, 0]
            pref[:, s] = (pref[:, s] << np.uint64(BITS)) | dig.astype(np.uint64)
    return pref


def np_mad(x, start, stop, window, center=None):
    """median(|float64(x) - center|) per window in numpy alone (center None: the window's median)."""
    wins = windows_of(x.shape[0], start, stop, window)
    cen = np_median(x, start, stop, window) if center is None else np.broadcast_to(np.asarray(center, np.float64), (len(wins), x.shape[1]))
    with np.errstate(invalid='ignore', over='ignore'):
        rows = [np.median(np.abs(x[a:b].astype(np.float64) - cen[w]), axis=0) for w, (a, b) in enumerate(wins)]
    return np.array(rows, np.float64).reshape(len(rows), x.shape[1])


def check_all(r, x, start, stop, window, channels, cols, q=(0.0, 0.25, 0.5, 0.999, 1.0), methods=('linear',)):
    """quantile (the methods given), median and mad of a Reader against the items x[:, cols] (x: what the file decodes to)."""
    xs = x[:, cols]
    i0 = r._validate_index(start, 0)
    i1 = max(i0, r._validate_index(stop, r.n_samples))
    one = isinstance(channels, (int, np.integer))                   # (an int channel drops the C axis: put it back for the comparison)
    for method in methods:
        got = r.quantile(list(q), start, stop, channels=channels, window=window, method=method)
        if one:
            assert got.quantile.ndim == 2
            got = dict(got, quantile=got.quantile[:, :, None], lower=got.lower[:, :, None], upper=got.upper[:, :, None])
            got = type('B', (), got)
        check_quantile(got, xs, i0, i1, window, q, method)
    med = r.median(start, stop, channels=channels, window=window)
    got = r.mad(start, stop, channels=channels, window=window)
    center, mad = got.center, got.mad
    if one:
        assert med.ndim == mad.ndim == center.ndim == 1
        med, mad, center = med[:, None], mad[:, None], center[:, None]
    assert same_values(med, np_median(xs, i0, i1, window)), ('median', window)
    assert same_values(center, med) and same_values(mad, np_mad(xs, i0, i1, window)), ('mad', window)
    assert got.count.tolist() == [b - a for a, b in windows_of(len(x), i0, i1, window)]
