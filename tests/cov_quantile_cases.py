"""The cases of tests/test_gpu_cov_quantile_edges.py (k_gram, k_gram_colsum, k_rank_hist on the MI355X) and of their CPU twins in
tests/test_cov_quantile_oracles.py (the numpy stand-ins GramOracleCodec / SelectOracleCodec / StatsOracleCodec): the inputs and the
checks are the same code, only the codec behind the Reader differs.  Every reference is the oracle's decode plus numpy, np.longdouble
or Python ints, never a device's output.

The recording: 2 * 4096 + 37 rows (two full slabs / tiles, one full 32-row step, then 5 rows: one whole 4-row MFMA block plus one row;
one 64-row unrolled pass of k_rank_hist plus a tail), 70 columns (two 64-column groups / super tiles, the second with 6 columns),
chunks of 1537 rows (boundaries inside 4-row blocks, 32-row steps and tiles).  The CPU twins pass a smaller shape: the stand-ins have
no tiles, and what they check is the references and the Reader's drivers."""
import numpy as np

import mtscomp_amd
from mtscomp_amd import hip
from tests.codec_oracle import OracleCodec
from tests.gram_oracle import assert_order_free, check_cov_result, exact_gram
from tests.select_oracle import check_all, check_quantile, np_mad, same_values
from tests.test_gpu_reduce_edges import value_families

DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']
ROWS, NC, CHUNK = 2 * 4096 + 37, 70, 1537
WINDOWS = (None, 4096, 4097, 999)
Q = (0.0, 0.25, 0.5, 0.999, 1.0)


def recording(tmp, x, chunk_rows, codec=None):
    """x written in chunks of chunk_rows rows.  -> (a Reader on `codec` (None: the device), what the oracle decodes: x, bit for bit)."""
    raw = tmp / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'd.cbin', tmp / 'd.ch', sample_rate=float(chunk_rows), n_channels=x.shape[1], dtype=x.dtype,
                         chunk_duration=1.0, do_time_diff=x.dtype.kind != 'f', check_after_compress=False, codec=codec)
    r = mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', codec=codec, check_after_decompress=False)
    ro = mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', codec=OracleCodec(), check_after_decompress=False)
    dec = ro[:]
    ro.close()
    assert dec.dtype == x.dtype and dec.tobytes() == x.tobytes()
    return r, dec


def grids(rows, nc):
    """(start, stop, window, channels) of every call: the four windows over the recording, a range that starts at row 3, and
    window=1 over 64 rows and a few columns of both column groups."""
    few = sorted({0, 1, 2, 3, nc - 1, nc // 2})
    windows = [w for w in WINDOWS if w is None or w < rows]          # (a shorter recording: windows beyond it are window None again)
    return [(0, rows, w, slice(None)) for w in windows] + [(3, rows, 4096, slice(None)), (rows // 2 - 30, rows // 2 + 34, 1, few)]


def _cols(channels, nc):
    return list(range(nc))[channels] if isinstance(channels, slice) else list(channels)


# ---- cov --------------------------------------------------------------------------------------------------------------------------
def cov_family(dtype, rows=ROWS, nc=NC):
    """value_families plus, for 8-byte integers, columns at the edges of the widening to double (columns 4..8: 2^53 + {0..7}, 2^63 - 1,
    ties between doubles spaced 1024 and 2048, 2^63 and 2^64 - 1 - {0, 1, 2} for uint64).  float64: the family's products overflow
    (column 1 is randn * 1e200, column 2 alternates +-max), and whether such an entry is finite, +-inf or NaN must not depend on the
    order of the sum or on fused arithmetic (assert_order_free checks that per call).  So column 1 and the odd columns from 3 on take
    the sign of column 2 in their row, the odd ones moved out of (0, 4) -- their products with +-max and with each other are 0 or
    overflow upwards: +inf --, and the even columns from 4 on are scaled by 2^-500: products with +-max stay near 1e160, squares near
    1e-297.  float32 items cannot overflow a double: as value_families gives them."""
    assert nc >= 10
    x = value_families(dtype, rows, nc, np.random.RandomState(100 + DTYPES.index(dtype)))
    dt, t = x.dtype, np.arange(rows)
    if dt.kind == 'f':                                                 # (+0 beside the family's -0: one key about the center 0.0)
        x[(t % 14 == 3) & np.isfinite(x[:, 0]), 0] = 0.0
    if dt == np.float64:
        sign = np.sign(x[:, 2])
        x[:, 1] = np.abs(x[:, 1]) * sign
        v = np.abs(x[:, 3::2])
        x[:, 3::2] = np.where((v != 0) & (v < 4), 4.0, v) * sign[:, None]
        x[:, 4::2] = np.ldexp(x[:, 4::2], -500)
    elif dt.itemsize == 8:
        x[:, 4] = ((1 << 53) + t % 8).astype(dt)
        x[:, 5] = np.array((1 << 63) - 1, dt)
        if dt.kind == 'i':
            x[:, 6] = -(1 << 53) - t % 8
            x[:, 7] = np.where(t % 2, (1 << 62) + 512, -(1 << 62) - 1536)            # halfway between two doubles
            x[:, 8] = np.iinfo(dt).min + t % 3
        else:
            x[:, 6] = np.uint64(1 << 63)
            x[:, 7] = np.uint64((1 << 64) - 1) - (t % 3).astype(np.uint64)
            x[:, 8] = np.uint64((1 << 63) + 1024) + (2048 * (t % 2)).astype(np.uint64)    # halfway: to the even neighbour
    return x


def run_cov(r, dec, teeth=True):
    """Reader.cov over every grid against check_cov_result (exact types bit for bit, sums of integers bit for bit, the others within
    the bound).  -> the largest error / allowance."""
    rows, nc = dec.shape
    worst = 0.0
    for start, stop, window, channels in grids(rows, nc):
        cols = _cols(channels, nc)
        if dec.dtype.kind == 'f':
            assert_order_free(dec[:, cols], start, stop, window)
        got = r.cov(start, stop, channels=channels, window=window)
        worst = max(worst, check_cov_result(got, dec[:, cols], start, stop, window, teeth=teeth))
    return worst


def small_ints(rows=ROWS, nc=NC, lo=-1024, hi=1024, seed=7):
    """k (rows, nc) int16 in [lo, hi] with both ends present in every window of 999 rows: |sum of products| < 2^34."""
    k = np.random.RandomState(seed).randint(lo, hi + 1, size=(rows, nc)).astype(np.int16)
    k[::500, 0], k[1::500, 0], k[::500, nc - 1] = lo, hi, hi
    return k


def run_scaled(r, k, e_cols, gram_bytes=True):
    """x[:, j] = k[:, j] * 2^e_cols[j] with every product and partial sum exactly representable: gram == ldexp(exact_gram(k), e_i +
    e_j) and sum == ldexp(sum k, e) by bytes, over every grid (integer items: sum in int64).  A flush of a subnormal operand or
    result anywhere in the kernel changes bytes here; no bound is involved."""
    rows, nc = k.shape
    e = np.broadcast_to(np.asarray(e_cols, np.int64), (nc,))
    for start, stop, window, channels in grids(rows, nc):
        cols = _cols(channels, nc)
        got = r.cov(start, stop, channels=channels, window=window)
        w = window or stop - start
        for i, a in enumerate(range(start, stop, w)):
            kw = k[a:min(a + w, stop)][:, cols]
            want = np.ldexp(exact_gram(kw).astype(np.float64), e[cols][:, None] + e[cols][None, :])
            assert got.gram.dtype == np.float64 and got.gram[i].tobytes() == want.tobytes(), (window, i, np.argwhere(got.gram[i] != want)[:4])
            s = kw.astype(np.int64).sum(0)
            if got.sum.dtype == np.int64:
                assert np.array_equal(got.sum[i], s << e[cols])
            else:
                assert got.sum[i].tobytes() == np.ldexp(s.astype(np.float64), e[cols]).tobytes(), (window, i)


def mixed_pair(k):
    """Even columns k * 2^-1074 (subnormal items), odd columns |k| * 2^900: the cross products k k' 2^-174 are normal and their sums
    exact, the even x even ones vanish (each is far below 2^-1075) and the odd x odd ones overflow upwards from the first non-zero
    product on.  -> (x, k with the odd columns' signs dropped, the exponents)."""
    odd = (np.arange(k.shape[1]) % 2).astype(bool)
    k = np.where(odd, np.abs(k), k)
    e = np.where(odd, 900, -1074)
    return np.ldexp(k.astype(np.float64), e), k, e


def run_mixed(r, x, k, e):
    rows, nc = k.shape
    odd = e > 0
    cross = odd[:, None] != odd[None, :]
    assert_order_free(x, 0, rows, None)                  # (no NaN or infinite items: what holds for all rows holds for any of them)
    for start, stop, window, channels in grids(rows, nc)[:-1]:
        got = r.cov(start, stop, window=window)
        w = window or stop - start
        for i, a in enumerate(range(start, stop, w)):
            G = exact_gram(k[a:min(a + w, stop)])
            with np.errstate(over='ignore'):
                want = np.ldexp(G.astype(np.float64), e[:, None] + e[None, :])
            g = got.gram[i]
            assert np.isfinite(want[cross]).all() and g[cross].tobytes() == want[cross].tobytes(), (window, i)
            assert (g[~odd][:, ~odd] == 0).all()
            assert np.array_equal(g[odd][:, odd], np.where(G[odd][:, odd] > 0, np.inf, 0.0)), (window, i)


def underflow_inexact(rows=ROWS, nc=NC):
    """float64 items whose squares are subnormal and round: (1 + rand) * 2e-162 in the first half of the columns, randn * 1e-310 in
    the second."""
    rs = np.random.RandomState(11)
    x = (1 + rs.rand(rows, nc)) * 2e-162
    x[:, nc // 2:] = rs.randn(rows, nc - nc // 2) * 1e-310
    return x


# ---- quantile / median / mad ----------------------------------------------------------------------------------------------------------
def centers(dec):
    """One center per column, by column % 4: 0 a value of the column (zero keys; for float column 0, 0.0 itself: -0 and +0 items give
    -0 and +0 differences, one key); 1 so large that x - c collapses to a few doubles (+-2^116, where doubles are 2^63 or 2^64 apart: every item of up to
    4 bytes gives one key, the 8-byte ones two or three); 2 NaN, +inf and -inf in turn; 3 a number between the items."""
    rows, nc = dec.shape
    c = np.empty(nc, np.float64)
    rs = np.random.RandomState(13)
    for j in range(nc):
        col = dec[:, j]
        fin = col[np.isfinite(col.astype(np.float64))]
        if j % 4 == 0:
            c[j] = 0.0 if dec.dtype.kind == 'f' and j == 0 else float(fin[len(fin) // 3])
        elif j % 4 == 1:
            c[j] = 2.0 ** 116 * (-1) ** (j // 4)
        elif j % 4 == 2:
            c[j] = (np.nan, np.inf, -np.inf)[(j // 4) % 3]
        else:
            c[j] = float(np.median(fin.astype(np.float64))) + rs.rand()
    return c


def run_quantile(r, dec, q=Q):
    """quantile / median / mad in key mode 0 over every grid through check_all, then modes 1 (x - c) and 2 (|x - c|) with `centers`
    through check_quantile, and mad about the same centers."""
    rows, nc = dec.shape
    cen = centers(dec)
    for start, stop, window, channels in grids(rows, nc):
        cols = _cols(channels, nc)
        check_all(r, dec, start, stop, window, channels, cols, q=q)
        for absolute in (False, True):
            got = r.quantile(list(q), start, stop, channels=channels, window=window, center=cen[cols], absolute=absolute, method='midpoint')
            check_quantile(got, dec[:, cols], start, stop, window, q, 'midpoint', mode=2 if absolute else 1, center=cen[cols])
        got = r.mad(start, stop, channels=channels, window=window, center=cen[cols])
        assert same_values(got.mad, np_mad(dec[:, cols], start, stop, window, center=cen[cols])), window


def divergence_family(dtype, rows=600, seed=0):
    """Two columns per key bit d of the item type: two values that differ at bit d only, half of the rows each, shuffled; and a cluster
    that shares every bit above d, random below, with three outliers.  The scan of a median must then walk down to the digit of bit
    d, and the columns of one wave are at different (prefix, shift) states in every round.  Float NaN patterns are replaced by 1.0."""
    dt = np.dtype(dtype)
    kb = 8 * dt.itemsize
    udt = np.dtype('uint%d' % kb)
    rs = np.random.RandomState(seed + kb)
    mask = (1 << kb) - 1
    cols = []
    for d in range(kb):
        base = int(rs.randint(0, 1 << 62)) & mask
        a = np.full(rows, base, dtype=np.uint64)
        a[rows // 2:] ^= np.uint64(1 << d)
        rs.shuffle(a)
        cols.append(a)
        low = np.uint64((1 << (d + 1)) - 1)
        b = (np.full(rows, base, dtype=np.uint64) & ~low) | (rs.randint(0, 1 << 62, rows).astype(np.uint64) & low)
        b[:3] = rs.randint(0, 1 << 62, 3).astype(np.uint64) & np.uint64(mask)
        cols.append(b)
    x = np.ascontiguousarray(np.stack(cols, axis=1).astype(udt)).view(dt)
    if dt.kind == 'f':
        x = np.where(np.isnan(x), dt.type(1.0), x).astype(dt)
    return np.ascontiguousarray(x)


def run_divergence(r, dec, windows=(None, 599, 200, 7)):
    rows, nc = dec.shape
    for window in windows:
        check_all(r, dec, 0, rows, window, slice(None), list(range(nc)), q=(0.0, 0.25, 0.5, 0.75, 1.0))
    got = r.mad()
    assert same_values(got.mad, np_mad(dec, 0, rows, None))
    return r.quantile(0.5).rounds, got.rounds


# ---- identities between the reductions --------------------------------------------------------------------------------------------
def run_consistency(r, dec):
    """Three kernels, one answer: cov().sum == window_stats().sum by bytes (integers), quantile(0 / 1).lower / upper ==
    window_stats().min / max (floats: windows without NaN, by value), float64(diag gram) == window_stats().sumsq by bytes (exact
    types).  Each side is held to its own reference elsewhere; this costs nothing more."""
    rows, nc = dec.shape
    ints = dec.dtype.kind in 'iu'
    for start, stop, window, channels in grids(rows, nc):
        cols = _cols(channels, nc)
        w = window or stop - start
        ws = r.window_stats(w, start, stop, channels=channels)
        qq = r.quantile([0.0, 1.0], start, stop, channels=channels, window=window)
        ok = np.ones(ws['min'].shape, bool) if ints else ~np.isnan(ws['min'].astype(np.float64)) & ~np.isnan(ws['max'].astype(np.float64))
        if not ints:                                                   # (a window with a NaN has a NaN min and max in window_stats)
            x = dec[:, cols]
            has_nan = np.array([np.isnan(x[a:min(a + w, stop)]).any(axis=0) for a in range(start, stop, w)])
            assert np.array_equal(ok, ~has_nan)
        assert qq.lower.dtype == ws['min'].dtype == dec.dtype
        assert same_values(qq.lower[:, 0][ok], ws['min'][ok]) and same_values(qq.upper[:, 1][ok], ws['max'][ok]), window
        if ints or hip.gram_exact(dec.dtype):
            cv = r.cov(start, stop, channels=channels, window=window)
            assert cv.sum.dtype == ws['sum'].dtype == np.int64 and cv.sum.tobytes() == np.ascontiguousarray(ws['sum']).tobytes(), window
            if hip.gram_exact(dec.dtype):
                diag = np.einsum('wii->wi', cv.gram).astype(np.float64)
                assert diag.tobytes() == np.ascontiguousarray(ws['sumsq']).tobytes(), window
