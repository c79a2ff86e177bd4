"""Test-only helpers for Reader.window_stats: the numpy definition of the statistics, and a lane codec that restates
mts_window_stats in numpy (so that the CPU suite drives the Python layer: argument handling, lanes, cache use, errors)."""
import math

import numpy as np

from tests.codec_oracle import LaneOracleCodec


def exact_sumsq(dtype):
    dtype = np.dtype(dtype)
    return dtype.kind in 'iu' and dtype.itemsize <= 2


def _identity(n_windows, n_cols, dtype):
    dtype = np.dtype(dtype)
    shape = (n_windows, n_cols)
    if dtype.kind == 'f':
        mn, mx = np.full(shape, np.inf, dtype), np.full(shape, -np.inf, dtype)
    else:
        mn, mx = np.full(shape, np.iinfo(dtype).max, dtype), np.full(shape, np.iinfo(dtype).min, dtype)
    s = np.zeros(shape, np.float64 if dtype.kind == 'f' else np.int64)
    q = np.zeros(shape, np.uint64 if exact_sumsq(dtype) else np.float64)
    return mn, mx, s, q


def segment_stats(x):
    """min, max, sum, sumsq of the rows of x (2-D) as the C ABI returns them (sumsq uint64 for 1/2-byte integers)."""
    if x.dtype.kind == 'f':
        return x.min(0), x.max(0), x.astype(np.float64).sum(0), (x.astype(np.float64) ** 2).sum(0)
    s = x.astype(np.int64).sum(0)
    if exact_sumsq(x.dtype):
        return x.min(0), x.max(0), s, (x.astype(np.int64) ** 2).sum(0).astype(np.uint64)
    return x.min(0), x.max(0), s, (x.astype(np.float64) ** 2).sum(0)


def numpy_window_stats(arr, window, start, stop, cols):
    """The contract: numpy over rows [start, stop) (already normalised) of the decoded array, columns `cols`.  `abssum`: the sum of
    |x| per window and column, the scale of the float tolerance."""
    cols = np.asarray(cols, dtype=np.int64)
    x = arr[start:stop][:, cols]
    n = stop - start
    nw = -(-n // window) if n > 0 else 0
    mn, mx, s, q = _identity(nw, cols.size, arr.dtype)
    cnt = np.zeros(nw, np.int64)
    abssum = np.zeros((nw, cols.size))
    for w in range(nw):
        seg = x[w * window:(w + 1) * window]
        cnt[w] = seg.shape[0]
        if cols.size:
            mn[w], mx[w], s[w], q[w] = segment_stats(seg)
            abssum[w] = np.abs(seg.astype(np.float64)).sum(0)
    sumsq = q.astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = s.astype(np.float64) / cnt[:, None]
        rms = np.sqrt(sumsq / cnt[:, None])
    return dict(count=cnt, min=mn, max=mx, sum=s, sumsq=sumsq, mean=mean, rms=rms, abssum=abssum)


def assert_stats_equal(got, want, dtype, squeeze=False):
    """min / max exactly (NaN where numpy has NaN; -0.0 == 0.0); integer sums and means bit for bit, the sums of squares too for
    1/2-byte integers; float64 accumulations within 1e-12 of the sum of |x| (resp. of x^2), NaN and +-inf where numpy has them."""
    dtype = np.dtype(dtype)
    assert got['count'].dtype == np.int64 and np.array_equal(got['count'], want['count'])
    exact = {'min', 'max'} | ({'sum', 'mean'} if dtype.kind != 'f' else set()) | ({'sumsq', 'rms'} if exact_sumsq(dtype) else set())
    cnt = np.maximum(want['count'], 1)[:, None]
    scale = dict(sum=want['abssum'], mean=want['abssum'] / cnt, sumsq=want['sumsq'], rms=want['rms'])
    for key in ('min', 'max', 'sum', 'sumsq', 'mean', 'rms'):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        sc = scale.get(key)
        if squeeze:
            w, sc = w[:, 0], (sc[:, 0] if sc is not None else None)
        assert g.shape == w.shape, (key, g.shape, w.shape)
        want_dt = dtype if key in ('min', 'max') else np.int64 if key == 'sum' and dtype.kind != 'f' else np.float64
        assert g.dtype == want_dt, (key, g.dtype, want_dt)
        if key in exact:
            assert np.array_equal(g, w, equal_nan=True), key
            continue
        assert np.array_equal(np.isnan(g), np.isnan(w)), key
        inf = np.isinf(w)
        assert np.array_equal(g[inf], w[inf]), key
        fin = np.isfinite(w)
        assert np.all(np.abs(g[fin] - w[fin]) <= 1e-12 * np.abs(sc[fin]) + 1e-300), key


class StatsOracleCodec(LaneOracleCodec):
    """LaneOracleCodec + window_stats restated in numpy: the partials of the given chunks (identities for windows they do not
    touch), resident chunks read from the lane's cache dict (E_MISS when a chunk without bytes is not there), the others
    decoded and NOT inserted.  Records (lane, keys, lens) of every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.stats_calls = []

    def window_stats(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, row_begin, row_end,
                     window_rows, cols, lane=None):
        dtype = np.dtype(dtype)
        self.stats_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens]))
        cols = np.asarray(cols, dtype=np.int64)
        assert window_rows >= 1 and cols.size and (cols >= 0).all() and (cols < n_channels).all()
        status, arrays = self._call_chunks('window_stats', cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags)
        nw = -(-(row_end - row_begin) // window_rows) if row_end > row_begin else 0
        mn, mx, s, q = _identity(nw, cols.size, dtype)
        cnt = np.zeros(nw, np.int64)
        for r0, nr, st, a in zip(row0, n_rows, status, arrays):
            assert r0 < row_end and r0 + nr > row_begin
            if st != 0:
                continue
            lo, hi = max(r0, row_begin), min(r0 + nr, row_end)
            r = lo
            while r < hi:
                w = (r - row_begin) // window_rows
                e = min(hi, row_begin + (w + 1) * window_rows)
                a_mn, a_mx, a_s, a_q = segment_stats(a[r - r0:e - r0][:, cols])
                mn[w], mx[w] = np.minimum(mn[w], a_mn), np.maximum(mx[w], a_mx)
                s[w] += a_s
                q[w] += a_q
                cnt[w] += e - r
                r = e
        return status, dict(min=mn, max=mx, sum=s, sumsq=q, count=cnt)


# ---- exact references: what the kernels' sums must come within a stated bound of -----------------------------------------------
STAT_TILE_ROWS = 512                     # reduce.hip: rows per tile of one (chunk ∩ window) segment
STAT_WAVES = 4                           # stats.hip: waves per tile, each taking every 4th row
U = 2.0 ** -53                           # unit roundoff of float64


def stat_tiles_per_window(chunk_bounds, start, stop, window):
    """(tiles of each window, rows of its largest tile): the tiling of reduce_plan.h's TilePlan for window_stats_run -- every (chunk ∩ window)
    segment of [start, stop) cut into STAT_TILE_ROWS-row tiles."""
    n = stop - start
    nw = -(-n // window) if n > 0 else 0
    tiles, big = np.zeros(nw, np.int64), np.zeros(nw, np.int64)
    b = np.asarray(chunk_bounds, np.int64)
    for i in range(b.size - 1):
        lo, hi = max(int(b[i]), start), min(int(b[i + 1]), stop)
        r = lo
        while r < hi:
            w = (r - start) // window
            e = min(hi, start + (w + 1) * window)
            tiles[w] += -(-(e - r) // STAT_TILE_ROWS)
            big[w] = max(big[w], min(e - r, STAT_TILE_ROWS))
            r = e
    return tiles, big


def stats_depth(chunk_bounds, start, stop, window, parts=1):
    """m per window: the longest chain of rounded float64 additions (and the rounded square) behind one result of a window.
    stats.hip:84-100 (k_stats_tiles): a lane adds every 4th row of its tile to an accumulator that starts at 0 -- at most
    ceil(min(tile rows, 512) / 4) additions -- and wave 0 then adds the 4 wave partials to 0 in wave order: 4 more.
    stats.hip:119-121 (k_stats_combine): the window's tile partials are added to 0 in tile order: one per tile.  A float64 item
    is squared with one rounding: 1 more.  `parts`: the partial results of lanes / device calls Reader.window_stats adds on the
    host (one addition each)."""
    tiles, big = stat_tiles_per_window(chunk_bounds, start, stop, window)
    return -(-big // STAT_WAVES) + STAT_WAVES + tiles + 1 + parts


def gamma(m):
    """gamma_m = m u / (1 - m u): |fl(sum) - sum| <= gamma_m * sum|terms| for any order of m - 1 rounded additions (Higham,
    Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.4) and Lemma 3.1)."""
    mu = np.asarray(m, np.float64) * U
    return mu / (1 - mu)


def _exact_sum(terms):
    """(value, sum of |terms|): math.fsum's correctly rounded sum where every term is finite and the sum stays in range; else the
    IEEE result of any order (NaN when a NaN or both infinities are there, the infinity otherwise; +-inf on overflow)."""
    t = np.asarray(terms, np.float64)
    a = float(np.abs(t).sum()) if t.size else 0.0
    if not np.isfinite(t).all():
        with np.errstate(invalid='ignore'):
            return float(t.sum()), a
    try:
        return math.fsum(t.tolist()), a
    except OverflowError:
        return (math.inf if t.sum() > 0 else -math.inf), a


def assert_stats_exact_bound(got, x, chunk_bounds, start, stop, window, cols, parts=1, squeeze=False):
    """got (Reader.window_stats / the C ABI's dict) against the exact sums of rows [start, stop) of x (the oracle's decode):
      floats:          |sum - fsum(x)| <= gamma_m * sum|x| and |sumsq - fsum(x^2)| <= gamma_m * sum x^2 with m = stats_depth (x^2
                       of a float32 item is exact in float64; of a float64 item it is rounded once, which m counts); NaN and
                       +-inf exactly where the terms make the exact sums NaN / +-inf; no bound where sum|terms| itself
                       overflows (then some partial sum overflows in almost any order: assert_stats_equal checks numpy's);
      4/8-byte ints:   sum == the Python-int sum wrapped to int64, bit for bit; |sumsq - sum x^2| <= (m + 3) u sum x^2 (the
                       exact Python-int sum of squares: each item converted to float64 (one rounding), squared (one), summed);
      1/2-byte ints:   sum and sumsq (uint64) exactly the Python-int sums.
    Returns the number of (window, column) results checked."""
    x = np.asarray(x)
    dtype = x.dtype
    cols = [int(c) for c in cols]
    m = stats_depth(chunk_bounds, start, stop, window, parts)
    s_got, q_got = np.asarray(got['sum']), np.asarray(got['sumsq'])
    if squeeze:
        s_got, q_got = s_got[:, None], q_got[:, None]
    nw = m.size
    assert s_got.shape == q_got.shape == (nw, len(cols)), (s_got.shape, nw, len(cols))
    for w in range(nw):
        seg = x[start + w * window:min(stop, start + (w + 1) * window)]
        for jc, c in enumerate(cols):
            col = seg[:, c]
            gs, gq = s_got[w, jc], q_got[w, jc]
            where = (w, jc, c)
            if dtype.kind == 'f':
                x64 = col.astype(np.float64)
                with np.errstate(over='ignore'):
                    sq = x64 * x64
                for name, g, terms in (('sum', gs, x64), ('sumsq', gq, sq)):
                    e, a = _exact_sum(terms)
                    if not np.isfinite(terms).all():
                        assert (math.isnan(g) and math.isnan(e)) or g == e, (name, where, g, e)
                        continue
                    if not math.isfinite(a):         # (sum |x| beyond float64: a partial sum may overflow in any order; no bound)
                        continue
                    assert math.isfinite(g) and abs(float(g) - e) <= float(gamma(m[w])) * a, (name, where, float(g), e, a, int(m[w]))
                continue
            ints = [int(v) for v in col.tolist()]
            s_exact = sum(ints)
            s_wrap = (s_exact + (1 << 63)) % (1 << 64) - (1 << 63)
            assert int(gs) == s_wrap, ('sum', where, int(gs), s_wrap)
            q_exact = sum(v * v for v in ints)
            if exact_sumsq(dtype):                       # (uint64 from the C ABI; Reader converts it to float64 once)
                want_q = q_exact if q_got.dtype == np.uint64 else float(q_exact)
                assert (int(gq) if q_got.dtype == np.uint64 else float(gq)) == want_q, ('sumsq', where, gq, q_exact)
            else:
                assert abs(float(gq) - q_exact) <= float(m[w] + 3) * U * q_exact, ('sumsq', where, float(gq), q_exact, int(m[w]))
    return nw * len(cols)
