"""Test-only restatement of mts_decimate in numpy: the FIR in the output dtype with the same operations in the same order as the
kernel (acc = 0, then acc = acc + taps[j] * x for j ascending, each rounded), and a lane codec built on it so that the CPU suite
drives Reader.decimate (argument handling, calls, lanes, cache use, errors) and can check bit-identity."""
import numpy as np

from tests.codec_oracle import LaneOracleCodec


def fir_decimate(x, x_row0, valid_begin, valid_end, first_row, n_out, q, taps, out_dtype):
    """y[k] = sum_j taps[j] * x[first_row + k * q - j] over the rows of x (2-D, file rows [x_row0, x_row0 + len(x))), 0 outside
    [valid_begin, valid_end), computed in out_dtype in the kernel's order."""
    out_dtype = np.dtype(out_dtype)
    xf = np.asarray(x).astype(out_dtype)
    tf = np.asarray(taps, dtype=np.float64).astype(out_dtype)
    acc = np.zeros((int(n_out), xf.shape[1]), out_dtype)
    rows = first_row + np.arange(int(n_out), dtype=np.int64) * q
    for j in range(tf.size):
        r = rows - j
        ok = (r >= valid_begin) & (r < valid_end)
        xr = np.zeros_like(acc)
        if ok.any():
            idx = r[ok] - x_row0
            assert idx.min() >= 0 and idx.max() < xf.shape[0], 'rows outside the chunks given'
            xr[ok] = xf[idx]
        with np.errstate(invalid='ignore', over='ignore'):
            acc = acc + tf[j] * xr
    return acc


def fir_decimate_f64(x, valid_begin, valid_end, first_row, n_out, q, taps):
    """The float64 reference and its scale: (y64, A) with A the same filter applied to |taps| and |x| (x: the whole recording, any
    dtype; only the rows the outputs read are converted)."""
    t = np.asarray(taps, dtype=np.float64)
    y = np.zeros((int(n_out), x.shape[1]))
    a = np.zeros_like(y)
    rows = first_row + np.arange(int(n_out), dtype=np.int64) * q
    for j in range(t.size):
        r = rows - j
        ok = (r >= valid_begin) & (r < valid_end)
        xr = np.zeros_like(y)
        xr[ok] = x[r[ok]].astype(np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            y += t[j] * xr
            a += abs(t[j]) * np.abs(xr)
    return y, a


def assert_within_bound(got, y64, a, n_taps, dtype):
    """|y - y64| <= (L + 4) * eps(dtype) * A where the reference is finite; NaN / inf where it has them."""
    eps = np.finfo(dtype).eps
    fin = np.isfinite(y64) & np.isfinite(a)
    g = np.asarray(got, dtype=np.float64)
    assert np.array_equal(np.isnan(g[~fin]), np.isnan(y64[~fin]))
    err = np.abs(g[fin] - y64[fin])
    bound = (n_taps + 4) * eps * a[fin] + np.finfo(dtype).tiny
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())


class DecimateOracleCodec(LaneOracleCodec):
    """LaneOracleCodec + decimate restated in numpy: resident chunks read from the lane's cache dict (E_MISS when a chunk without
    bytes is not there), the others decoded and NOT inserted.  Records (lane, keys, lens) of every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.decimate_calls = []

    def decimate(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, first_row, n_out, q,
                 taps, out_dtype, cols, lane=None):
        dtype = np.dtype(dtype)
        self.decimate_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens]))
        cols = np.asarray(cols, dtype=np.int64)
        assert q >= 1 and cols.size and (cols >= 0).all() and (cols < n_channels).all()
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        status, arrays = self._call_chunks('decimate', cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols] if arrays else np.zeros((0, cols.size), dtype)
        y = fir_decimate(x, int(row0[0]) if len(keys) else 0, valid_begin, valid_end, first_row, n_out, q, taps, out_dtype)
        return status, y


# ---- an exact reference that shares nothing with the kernel but the formula (decimate.hip:3) -------------------------------------
MANTISSA_BITS = {4: 24, 8: 53}


def exact_tap_budget(x_max, out_dtype):
    """The largest sum of |k_j| for which dyadic taps k_j / 2^s on integer items |x| <= x_max give exact results in out_dtype.
    With p mantissa bits (24 for float32, 53 for float64): an item (|x| <= x_max < 2^p) and a tap (|k_j| < 2^p) are exact in the
    output type, every product k_j x / 2^s is an integer times 2^-s of magnitude below 2^p / 2^s, and so is every partial sum,
    as long as sum_j |k_j| * x_max <= 2^p: then each product and each sum is exactly representable and no rounding happens
    anywhere, in any order.  (2^-s stays far above the smallest subnormal for the s used here.)"""
    p = MANTISSA_BITS[np.dtype(out_dtype).itemsize]
    return (1 << p) // max(int(x_max), 1)


def dyadic_taps(rs, n_taps, budget, max_shift=20):
    """(k, s, taps): n_taps random integers k (sum |k| <= budget, k[0] and k[-1] nonzero so that the first and last tap both
    count) and taps = k / 2^s, exact in float64."""
    kmax = max(1, budget // n_taps)
    k = rs.randint(-kmax, kmax + 1, size=n_taps).astype(np.int64)
    k[0] = k[0] or 1
    k[-1] = k[-1] or -1
    while np.abs(k).sum() > budget:                        # (only when kmax == 1 and the ends were bumped)
        nz = np.flatnonzero(k[1:-1]) + 1
        k[nz[0]] = 0
    s = int(rs.randint(0, max_shift + 1))
    return k, s, k.astype(np.float64) / float(1 << s)


def fir_decimate_exact(x, x_row0, valid_begin, valid_end, first_row, n_out, q, k, s, out_dtype):
    """sum_j k_j * x[first_row + i q - j] / 2^s in int64 integers (x: integer items, or floats holding integers), 0 outside
    [valid_begin, valid_end), then scaled by 2^-s and converted to out_dtype -- exactly, when sum |k| * max|x| <= 2^p
    (exact_tap_budget): asserted here."""
    xi = np.asarray(x)
    assert xi.dtype.kind in 'iu' or np.array_equal(xi, np.round(xi)), 'items are not integers'
    xi = xi.astype(np.int64)
    k = np.asarray(k, np.int64)
    x_max = int(np.abs(xi).max()) if xi.size else 0
    assert int(np.abs(k).sum()) * x_max <= 1 << MANTISSA_BITS[np.dtype(out_dtype).itemsize], 'not exactly representable'
    acc = np.zeros((int(n_out), xi.shape[1]), np.int64)
    rows = first_row + np.arange(int(n_out), dtype=np.int64) * q
    for j in np.flatnonzero(k):
        r = rows - j
        ok = (r >= valid_begin) & (r < valid_end)
        if ok.any():
            idx = r[ok] - x_row0
            assert idx.min() >= 0 and idx.max() < xi.shape[0], 'rows outside the chunks given'
            acc[ok] += k[j] * xi[idx]
    return (acc.astype(np.float64) / float(1 << s)).astype(out_dtype)       # (|acc| <= 2^53: both conversions exact)


# ---- the launch plan of k_decimate, restated (decimate.hip:162-174) ------------------------------------------------------------
DEC_LDS_BYTES = 65536
DEC_SLAB_MAX = 64


def dec_plan(n_taps, q, out_dtype):
    """(S, R, tile_out, slab) as dec_plan<F> chooses them: S ring rows, R outputs per lane, tile_out outputs per workgroup, slab
    taps staged per step."""
    S = DEC_LDS_BYTES // (64 * np.dtype(out_dtype).itemsize)
    want = min(n_taps, 32)
    to = min((S - want) // q + 1, 64)
    R = 8 if to >= 64 else 4 if to >= 32 else 2 if to >= 16 else 1
    tile_out = min(to, 8 * R)
    slab = min(S - (tile_out - 1) * q, DEC_SLAB_MAX)
    return S, R, tile_out, slab


def plan_branches(n_taps, q, out_dtype, n_out=None):
    """The names of the plan branches (q, L, out_dtype[, n_out]) reaches, as listed in the tests' coverage assertion."""
    S, R, to, slab = dec_plan(n_taps, q, out_dtype)
    f = 'f%d' % (8 * np.dtype(out_dtype).itemsize)
    b = {'R=%d/%s' % (R, f), 'slab==64' if slab == DEC_SLAB_MAX else 'slab<64'}
    if to == 1:
        b.add('tile_out==1')
    if n_taps == 1:
        b.add('L==1')
    b.add('L<=slab' if n_taps <= slab else 'L>slab')
    for d, name in ((-1, 'S-1'), (0, 'S'), (1, 'S+1')):
        if n_taps == S + d:
            b.add('L==%s/%s' % (name, f))
    if n_taps == 8192:
        b.add('L==8192/%s' % f)
    if q == 1:
        b.add('q==1')
    if q >= S:
        b.add('q>=S/%s' % f)
    if n_out is not None and to > 1:
        r = n_out % to
        b |= {'n_out%%tile==%s' % name for v, name in ((0, '0'), (1, '1'), (to - 1, 'tile-1')) if r == v}
    return b


PLAN_BRANCHES = ({'R=%d/%s' % (r, f) for r in (1, 2, 4, 8) for f in ('f32', 'f64')}
                 | {'tile_out==1', 'slab<64', 'slab==64', 'L==1', 'L<=slab', 'L>slab', 'q==1'}
                 | {'%s/%s' % (n, f) for n in ('L==S-1', 'L==S', 'L==S+1', 'L==8192', 'q>=S') for f in ('f32', 'f64')}
                 | {'n_out%tile==0', 'n_out%tile==1', 'n_out%tile==tile-1'})

# (q, n_taps, out dtype): every branch of PLAN_BRANCHES but the n_out residues, which the tests take per call
DECIMATE_PLAN_CASES = [
    (2, 16, 'float32'), (1, 5, 'float32'), (3, 1, 'float32'), (5, 32, 'float32'), (12, 241, 'float32'), (40, 3, 'float32'),
    (256, 8192, 'float32'), (300, 1, 'float32'), (7, 255, 'float32'), (3, 256, 'float32'), (64, 257, 'float32'),
    (224, 33, 'float32'), (225, 33, 'float32'),
    (1, 7, 'float64'), (2, 2, 'float64'), (2, 1, 'float64'), (2, 32, 'float64'), (3, 9, 'float64'), (5, 16, 'float64'),
    (12, 241, 'float64'), (20, 9, 'float64'), (96, 40, 'float64'), (97, 129, 'float64'), (128, 8192, 'float64'),
    (4, 127, 'float64'), (1, 128, 'float64'), (400, 3, 'float64'),
]


def plan_n_outs(n_taps, q, out_dtype):
    """n_out values that put n_out mod tile_out at 0, 1 and tile_out - 1 (one value when tile_out == 1)."""
    to = dec_plan(n_taps, q, out_dtype)[2]
    return sorted({v for v in (to, to + 1, 2 * to - 1) if v >= 1}) if to > 1 else [2]
