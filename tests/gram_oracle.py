"""Test-only restatements of mts_gram in numpy: the groups of Reader.cov's grid (exact types: int64 Gram entries from float64 BLAS over
blocks of at most 2^20 rows; float types: float64 per group, groups added in order), a lane codec built on it so that the CPU suite
drives Reader.cov (argument handling, calls, lanes, cache use, errors), a reference in np.longdouble, and the error bounds the GPU
results are held to: gram_bound for the Gram entries (the height of the tree include/mtscomp_hip.h documents, plus the absolute
underflow term derived below) and cov_bound for the covariance formula.

Underflow.  With gradual underflow the standard model of a float64 operation gains an absolute term for products only:
fl(a * b) = a * b * (1 + d) + e and fl(a * b + c) = (a * b + c) * (1 + d) + e with |d| <= u, |e| <= 2^-1075 (half the smallest subnormal;
e != 0 only when the result is subnormal, and then d = 0), while fl(a + b) needs no e at all: a sum of two doubles that lands in the
subnormal range is a multiple of 2^-1074 below 2^-1022 and therefore exact.  A Gram entry of a window of n rows holds n products, each
rounded once where it is formed (alone or fused with the running sum), so at most n such e enter it; the h later roundings of the tree
scale each by at most 1 + gamma_h < 2.  The sum of |x_ti x_tj| the relative term is taken from is itself computed in float64 and may fall
short of the true one by n * 2^-1075, which moves the relative term by less than gamma_{h+3} * n * 2^-1075.  Together: an absolute
allowance of n * 2^-1075 * (1 + gamma_h + gamma_{h+3}) <= n * 2^-1074 = underflow_term(n).  The new bound is the old one plus that
term and nothing else; wherever the sum of |x_ti x_tj| reaches n * 2^-1021 (1e-303 for a window of 2^20 rows) the term is below u times
that sum, one of the h + 3 units of the relative part.  The longdouble reference has a 15-bit exponent and does not underflow on
float64 items.  (A kernel that flushed subnormal operands or results to zero would need n * 2^-1022 per flushed product instead; the
exact scaled-integer cases of tests/cov_quantile_cases.py show by bytes that k_gram does not.)"""
from fractions import Fraction

import numpy as np

from mtscomp_amd import hip
from tests.codec_oracle import LaneOracleCodec

U = 2.0 ** -53                                 # unit roundoff of float64
UL = 2.0 ** -64                                # ... of np.longdouble with a 64-bit mantissa


def gamma(k, u=U):
    return k * u / (1 - k * u)


def widen(x):
    """The items as the kernel sees them: converted to float64 once (exact but for 8-byte integers, which are rounded)."""
    return np.asarray(x).astype(np.float64)


def exact_gram(x):
    """x.astype(int64).T @ x.astype(int64) with numpy's wrap, for 1- and 2-byte integers: float64 BLAS over blocks of <= 2^20 rows
    (every partial sum is an integer below 2^52, so the blocks are exact), each converted to int64, then added with wrap."""
    x = np.asarray(x)
    out = np.zeros((x.shape[1], x.shape[1]), np.int64)
    for r in range(0, x.shape[0], 1 << 20):
        b = x[r:r + (1 << 20)].astype(np.float64)
        out += (b.T @ b).astype(np.int64)
    return out


def group_partial(x):
    """(gram, sum) of one group's items x (rows, n_cols) in gram_dtypes: exact types bit for bit; float types in float64 (BLAS: the
    stand-in's order, not the kernel's)."""
    x = np.array(x, order='C', copy=True)           # (a fresh array: BLAS and numpy's sums give the same bits whatever the view)
    g_dt, s_dt = hip.gram_dtypes(x.dtype)
    if hip.gram_exact(x.dtype):
        g = exact_gram(x)
    else:
        xf = widen(x)
        with np.errstate(invalid='ignore', over='ignore'):
            g = xf.T @ xf
    if x.dtype.kind == 'f':
        with np.errstate(invalid='ignore', over='ignore'):
            s = widen(x).sum(axis=0)
    else:
        s = x.astype(np.int64).sum(axis=0)           # (modulo 2^64, as the kernel's u64 sums; uint64 items reinterpreted)
    return g.astype(g_dt), s.astype(s_dt)


def gram_partials(x, x_row0, range_begin, range_end, window, g0, g1):
    """The partials mts_gram returns for groups [g0, g1) of the grid, x: 2-D items (columns already chosen) holding file rows
    [x_row0, x_row0 + len(x)).  -> (gram (n, C, C), sum (n, C))."""
    g_dt, s_dt = hip.gram_dtypes(x.dtype)
    n = g1 - g0
    G = np.zeros((n, x.shape[1], x.shape[1]), g_dt)
    S = np.zeros((n, x.shape[1]), s_dt)
    for j in range(n):
        lo, hi = hip.gram_group_rows(range_begin, range_end, window, g0 + j)
        assert x_row0 <= lo and hi <= x_row0 + x.shape[0], 'rows outside the chunks given'
        G[j], S[j] = group_partial(x[lo - x_row0:hi - x_row0])
    return G, S


def window_grams(x, start, stop, window):
    """Reader.cov's gram and sum per window from the groups, added in group order (int64 with wrap; float64 from +0)."""
    window = window or max(stop - start, 1)
    n_win = -(-(stop - start) // window)
    g_dt, s_dt = hip.gram_dtypes(x.dtype)
    G = np.zeros((n_win, x.shape[1], x.shape[1]), g_dt)
    S = np.zeros((n_win, x.shape[1]), s_dt)
    K = -(-window // hip.GRAM_GROUP_ROWS)
    for g in range(hip.gram_groups(start, stop, window) if n_win else 0):
        lo, hi = hip.gram_group_rows(start, stop, window, g)
        a, b = group_partial(x[lo:hi])
        G[g // K] += a
        S[g // K] += b
    return G, S


class GramOracleCodec(LaneOracleCodec):
    """LaneOracleCodec + gram restated in numpy: resident chunks read from the lane's cache dict (E_MISS when a chunk without bytes is
    not there), the others decoded and NOT inserted.  Records (lane, keys, lens, group_begin, group_end) of every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.gram_calls = []

    def gram(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, range_begin, range_end, window_rows, group_begin,
             group_end, cols, lane=None):
        dtype = np.dtype(dtype)
        self.gram_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(group_begin), int(group_end)))
        cols = np.asarray(cols, dtype=np.int64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all()
        assert 0 <= group_begin < group_end <= hip.gram_groups(range_begin, range_end, window_rows)
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        status, arrays = self._call_chunks('gram', cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        G, S = gram_partials(x, int(row0[0]), range_begin, range_end, window_rows, group_begin, group_end)
        return status, G, S


# ---- the reference and the bounds ----------------------------------------------------------------------------------------------------
def tree_height(n_rows_window):
    """h of include/mtscomp_hip.h for a window of n rows: inside a group of m rows a product goes through at most min(m, SLAB) +
    ceil(m / SLAB) - 1 roundings (the MFMA chain of its slab, then the slabs in order); the host adds the window's groups in order."""
    n = int(n_rows_window)
    GR, SR = hip.GRAM_GROUP_ROWS, hip.GRAM_SLAB_ROWS
    groups = [min(GR, n - r) for r in range(0, n, GR)]
    inner = max(min(m, SR) + -(-m // SR) - 1 for m in groups) if groups else 0
    return inner + max(len(groups) - 1, 0)


TINY = 2.0 ** -1074                            # the smallest float64 subnormal


def underflow_term(n_rows):
    """n * 2^-1074: what n products rounded in the subnormal range can add to a Gram entry (the module's docstring derives it)."""
    return np.asarray(n_rows, np.float64) * TINY


def gram_bound(h, absgram, n_rows=0):
    """|G - sum_t x_ti x_tj| <= gamma_{h+3} * sum_t |x_ti x_tj| + n_rows * 2^-1074 for a tree of height h over n_rows rows (absgram:
    computed in float64 from |x|).  n_rows = 0 is the purely relative bound, which holds only where no product is subnormal."""
    return gamma(h + 3) * absgram + underflow_term(n_rows)


def reference(x):
    """(sum_t x_ti x_tj in np.longdouble, its own error bound, sum_t |x_ti x_tj| in float64) of the widened items."""
    xf = widen(x)
    xl = xf.astype(np.longdouble)
    ref = xl.T @ xl
    a = np.abs(xf)
    absgram = a.T @ a
    n = xf.shape[0]
    return ref, (n + 2) * UL * absgram, absgram


def gram_allowance(x, h):
    """The allowance of a float Gram against `reference`: gram_bound(h) + the reference's own error.  -> (ref, allowance)."""
    ref, ref_err, absgram = reference(x)
    return ref, gram_bound(h, absgram, np.asarray(x).shape[0]) + ref_err


def assert_gram_within(got, x, h):
    """got (C, C) float64 within gram_bound of the longdouble reference (finite entries), and the bound has teeth: removing any
    single row of x would move some entry of the exact Gram by more than the allowance."""
    ref, allow = gram_allowance(x, h)
    err = np.abs(got.astype(np.longdouble) - ref)
    assert (err <= allow).all(), 'max err / allowance %.3g' % float((err / np.maximum(allow, TINY)).max())
    xf = widen(x)
    outer_diag = xf * xf                                     # row t's contribution to the diagonal entries
    assert (outer_diag > np.diag(allow)[None, :]).any(axis=1).all(), 'a row whose removal the bound would not catch'
    return float((err / np.maximum(allow, TINY)).max())


def assert_order_free(x, start, stop, window):
    """Whether an entry of the Gram of x (float items, the columns chosen) is finite, +-inf or NaN must depend neither on the order of
    its sum nor on whether a product is rounded before it is added (a fused multiply-add sees the finite product 1e400 where the
    separate multiplication sees +inf: -inf + 1e400 is -inf fused and NaN unfused), or no reference could say what the kernel owes.
    Per window and entry, with the products formed in np.longdouble (which holds them all):
      * a NaN product (a NaN item, inf * 0) makes the entry NaN whatever the arithmetic;
      * a product is `huge` when it is infinite or at least 2 * max in magnitude (infinite even when fused with a finite addend of
        the other sign); the huge products of an entry must all have one sign (the entry is that infinity), unless infinite items
        alone give both signs (NaN, fused or not);
      * all other products are finite, and the sum of their magnitudes must stay below max / 2: no partial sum overflows.
    A case that fails here needs other inputs, not a skipped check.  (Only entries with a column that holds a non-finite item or one
    beyond 2^500 are walked: among the others a window of fewer than 2^20 rows sums to less than 2^1020.)"""
    fmax = np.longdouble(np.finfo(np.float64).max)
    w = window or max(stop - start, 1)
    assert w < 1 << 20
    with np.errstate(invalid='ignore'):
        hot = np.flatnonzero(~(np.abs(widen(x[start:stop])) <= 2.0 ** 500).all(axis=0))
    for a in range(start, stop, w):
        xl = widen(x[a:min(a + w, stop)]).astype(np.longdouble)
        for i in hot:
            with np.errstate(invalid='ignore', over='ignore'):
                p = xl[:, i:i + 1] * xl
            nan = np.isnan(p)
            huge = ~nan & (np.abs(p) >= 2 * fmax)
            both = (huge & (p > 0)).any(axis=0) & (huge & (p < 0)).any(axis=0)
            both_inf = (np.isposinf(p)).any(axis=0) & (np.isneginf(p)).any(axis=0)
            rest = np.where(nan | huge, 0, np.abs(p)).sum(axis=0)
            ok = nan.any(axis=0) | both_inf | (~both & (rest < fmax / 2))
            assert ok.all(), 'window at row %d, entries (%d, %s): the order of the sum decides' % (a, i, np.flatnonzero(~ok)[:5].tolist())


def cov_exact(G, s, n, ddof):
    """(n G - s s^T) / (n (n - ddof)) as Fractions of the given (exact or returned) G and s."""
    C = len(s)
    out = np.empty((C, C), object)
    sf = [Fraction(int(v)) if isinstance(v, (int, np.integer)) else Fraction(float(v)) for v in s]
    for i in range(C):
        for j in range(C):
            g = G[i, j]
            gf = Fraction(int(g)) if isinstance(g, (int, np.integer)) else Fraction(float(g))
            out[i, j] = (n * gf - sf[i] * sf[j]) / (n * (n - ddof))
    return out


def cov_bound(G, s, n, ddof, gram_err=0.0):
    """(count - ddof) |c_hat - c| <= 7u (|G_ij| + |s_i s_j| / count) (+ the Gram's own error for float types): the allowance per
    entry, divided by count - ddof."""
    Gf = np.abs(np.asarray(G, dtype=np.float64))
    sf = np.asarray(s, dtype=np.float64)
    return (7 * U * (Gf + np.abs(np.outer(sf, sf)) / n) + gram_err) / (n - ddof)


def assert_cov_exact_bound(c, G, s, n, ddof):
    """c (C, C) float64 within cov_bound of the exact rational of (G, s)."""
    want = cov_exact(G, s, n, ddof)
    bound = cov_bound(G, s, n, ddof)
    worst = 0.0
    for i in range(len(s)):
        for j in range(len(s)):
            e = abs(Fraction(float(c[i, j])) - want[i, j])
            assert e <= Fraction(float(bound[i, j])), (i, j, float(e), bound[i, j])
            worst = max(worst, float(e) / bound[i, j] if bound[i, j] else 0.0)
    return worst


def _windows(x, start, stop, window):
    """x[start:stop] as (n_win, w, C) with the last window padded with zeros, and the rows per window."""
    w = window or max(stop - start, 1)
    n_win = -(-(stop - start) // w)
    xs = x[start:stop]
    pad = np.zeros((n_win * w, x.shape[1]), x.dtype)
    pad[:stop - start] = xs
    counts = np.minimum(w, (stop - start) - w * np.arange(n_win))
    return pad.reshape(n_win, w, x.shape[1]), counts


def check_cov_result(got, x, start, stop, window, ddof=1, teeth=True):
    """Reader.cov's result against the items x (the columns already chosen, the decoded recording): count; exact types bit for bit
    against numpy int64 (gram and sum); other types' Gram entries within gram_bound of the longdouble reference with h from the
    header's tree (finite references only; NaN and +-inf exactly where the float64 reference has them) and the bound's teeth; float
    sums within gamma_{h+1} sum |x| (+ the reference's own error); G == G^T bitwise; mean and cov as the formula.  -> the largest
    error / allowance of the float Gram entries (0 for exact types).  teeth=False skips the teeth (random data may hold a row of
    near-zero items whose removal no bound of this form can see: the fuzzer's)."""
    X, counts = _windows(x, start, stop, window)
    assert got.count.tolist() == counts.tolist()
    C = x.shape[1]
    assert got.gram.shape == (len(counts), C, C) and got.sum.shape == (len(counts), C)
    assert np.array_equal(got.gram, np.swapaxes(got.gram, 1, 2), equal_nan=True)
    assert got.gram.tobytes() == np.ascontiguousarray(np.swapaxes(got.gram, 1, 2)).tobytes()
    worst = 0.0
    if x.dtype.kind in 'iu':
        assert np.array_equal(got.sum, X.astype(np.int64).sum(axis=1))
    if hip.gram_exact(x.dtype):
        Xi = X.astype(np.int64)
        assert np.array_equal(got.gram, np.swapaxes(Xi, 1, 2) @ Xi)
    else:
        Xf = widen(X)
        A = np.abs(Xf)
        with np.errstate(invalid='ignore', over='ignore'):
            absgram = np.swapaxes(A, 1, 2) @ A
            Xl = Xf.astype(np.longdouble)
            ref = np.swapaxes(Xl, 1, 2) @ Xl
            ref64 = np.swapaxes(Xf, 1, 2) @ Xf
        h = np.array([tree_height(c) for c in counts], np.float64)
        gam = (h + 3) * U / (1 - (h + 3) * U)
        allow = gam[:, None, None] * absgram + (counts + 2)[:, None, None] * UL * absgram + underflow_term(counts)[:, None, None]
        fin = np.isfinite(absgram)
        g = got.gram
        assert np.array_equal(np.isnan(g), np.isnan(ref64))
        assert np.array_equal(np.isposinf(g), np.isposinf(ref64)) and np.array_equal(np.isneginf(g), np.isneginf(ref64))
        err = np.abs(g.astype(np.longdouble) - ref)
        ok = np.where(fin, err <= allow, True)
        if not ok.all():
            w, i, j = np.argwhere(~ok)[0]
            raise AssertionError('gram[%d, %d, %d] = %r, reference %r, allowance %r' % (w, i, j, g[w, i, j], float(ref[w, i, j]), allow[w, i, j]))
        if fin.any():
            worst = float(np.max(np.where(fin, err / np.maximum(allow, TINY), 0)))
        # teeth: in a window of finite items, every row with a nonzero item would, if dropped, move a diagonal entry by more than its
        # allowance (windows that hold NaN or +-inf are checked for where those land, and the finite entries for the bound)
        d = np.einsum('wii->wi', allow)
        sq = Xf * Xf
        live = (Xf != 0).any(axis=2) & np.isfinite(Xf).all(axis=(1, 2))[:, None]
        caught = (sq > d[:, None, :]).any(axis=2)
        assert not teeth or caught[live].all(), 'a row whose removal the bound would not catch'
        if x.dtype.kind == 'f':
            with np.errstate(invalid='ignore', over='ignore'):
                sref = Xl.sum(axis=1)
                sabs = A.sum(axis=1)
            sfin = np.isfinite(sabs)
            sallow = ((h + 1) * U / (1 - (h + 1) * U))[:, None] * sabs + (counts + 2)[:, None] * UL * sabs
            serr = np.abs(got.sum.astype(np.longdouble) - sref)
            assert np.where(sfin, serr <= sallow, True).all()
    with np.errstate(invalid='ignore', divide='ignore'):
        sf = got.sum.astype(np.float64)
        mean = sf / got.count[:, None]
        want = (got.gram.astype(np.float64) - sf[:, :, None] * mean[:, None, :]) / (got.count - ddof)[:, None, None]
    want[got.count - ddof <= 0] = np.nan
    assert got.cov.tobytes() == want.tobytes() and got.mean.tobytes() == mean.tobytes()
    return worst
