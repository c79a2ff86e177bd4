"""Test-only restatements of mts_project in numpy: the float32 definition (the fmaf chain of include/mtscomp_hip.h, with an exact
vectorised fmaf), a reference in np.longdouble with its own error, the bound the float64 results are held to, and a lane codec built
on them so that the CPU suite drives Reader.project (argument handling, calls, lanes, cache use, errors) and can check bit-identity.

The bound.  With F the compute type, u its unit roundoff (2^-24 or 2^-53), tiny its smallest subnormal (2^-149 or 2^-1074) and n4 =
n_cols rounded up to a multiple of 4, a term (x_j - o_j) w_jk of output y[t, k] goes through these roundings: the conversion of the item
and of the offset to F (one factor (1 + d) on each of x_j and o_j), the subtraction (one), the conversion of the weight (one), and the
chain: a 4-column matrix step rounds a term at most 4 times (bit for bit one fma per column for float32), so at most n4 in all.  That
is (|x_j| + |o_j|) |w_jk| (1 + d)^(n4 + 3) at worst, hence, with gamma_k = k u / (1 - k u),

    |y - sum_j (x_j - o_j) w_jk| <= gamma_{n4+4} * sum_j (|x_j| + |o_j|) |w_jk| + n4 * tiny.

The absolute term is the gradual underflow, as in tests/gram_oracle.py: each of the at most n4 products may be rounded in the subnormal
range (an error of at most tiny / 2, scaled by less than 2 by the later roundings); sums that land there are exact.  The bound assumes
that no conversion to F overflows or underflows (the tests' items, offsets and weights are chosen so), and it is compared where the
reference is finite.  The reference forms the same sum in np.longdouble (64-bit mantissa: every item type is exact in it); its own
error, (n_cols + 2) * 2^-64 * sum_j (|x_j| + |o_j|) |w_jk|, is added to the allowance."""
import numpy as np

from tests.codec_oracle import LaneOracleCodec

UL = 2.0 ** -64                                # unit roundoff of np.longdouble with a 64-bit mantissa
UNIT = {4: 2.0 ** -24, 8: 2.0 ** -53}
TINY = {4: 2.0 ** -149, 8: 2.0 ** -1074}


def gamma(k, u):
    return k * u / (1 - k * u)


def fmaf_f32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, exactly: the product of two float32 is exact in float64; the float64 sum with c is taken with
    its TwoSum error and, when that error is not zero and the sum's last bit is even, moved to its odd neighbour on the error's side
    (round to odd); one rounding to float32 follows.  53 >= 24 + 2 bits, so the double rounding is innocuous."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        even = (s.view(np.int64) & 1) == 0
        move = np.isfinite(s) & even & (err != 0)                  # (a NaN err compares unequal: masked by isfinite(s) and p, c below)
        move &= np.isfinite(p) & np.isfinite(c64)
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(move, odd, s).astype(np.float32)


def _converted(x, offset, weights, dtype):
    """(d, w) as the kernel forms them: items, offsets and weights each rounded once to `dtype`, d = x - o in it; padded to n4."""
    dtype = np.dtype(dtype)
    x = np.asarray(x)
    w = np.asarray(weights, dtype=np.float64)
    n_cols = x.shape[1]
    assert w.shape[0] == n_cols
    o = np.zeros(n_cols) if offset is None else np.broadcast_to(np.asarray(offset, dtype=np.float64), (n_cols,))
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        d = x.astype(dtype) - o.astype(dtype)[None, :]
        wf = w.astype(dtype)
    n4 = -(-n_cols // 4) * 4
    d = np.concatenate([d, np.zeros((x.shape[0], n4 - n_cols), dtype)], axis=1)
    wf = np.concatenate([wf, np.zeros((n4 - n_cols, w.shape[1]), dtype)], axis=0)
    return d, wf


def project_chain_f32(x, offset, weights):
    """The float32 definition of mts_project on items x (rows, n_cols; the columns already chosen): acc = +0, then
    acc = fmaf(d[:, j], w[j, :], acc) for j = 0 .. n4 - 1."""
    d, w = _converted(x, offset, weights, np.float32)
    acc = np.zeros((d.shape[0], w.shape[1]), np.float32)
    for j in range(d.shape[1]):
        acc = fmaf_f32(d[:, j:j + 1], w[j:j + 1, :], acc)
    return acc


def project_chain_f64(x, offset, weights):
    """A float64 stand-in for the CPU suite: acc = acc + d[:, j] * w[j, :] for j ascending (two roundings a step: the stand-in's
    arithmetic, not the matrix cores'; a row's result depends on that row alone, which is what the host logic needs)."""
    d, w = _converted(x, offset, weights, np.float64)
    acc = np.zeros((d.shape[0], w.shape[1]), np.float64)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        for j in range(d.shape[1]):
            acc = acc + d[:, j:j + 1] * w[j:j + 1, :]
    return acc


def project_chain(x, offset, weights, dtype):
    return project_chain_f32(x, offset, weights) if np.dtype(dtype).itemsize == 4 else project_chain_f64(x, offset, weights)


def project_reference(x, offset, weights):
    """(sum_j (x_j - o_j) w_jk in np.longdouble, its own error bound, sum_j (|x_j| + |o_j|) |w_jk| in float64) of the items as they
    are (no conversion: every item type is exact in longdouble)."""
    x = np.asarray(x)
    w = np.asarray(weights, dtype=np.float64)
    n_cols = x.shape[1]
    o = np.zeros(n_cols) if offset is None else np.broadcast_to(np.asarray(offset, dtype=np.float64), (n_cols,))
    xl, ol, wl = x.astype(np.longdouble), o.astype(np.longdouble), w.astype(np.longdouble)
    with np.errstate(invalid='ignore', over='ignore'):
        ref = (xl - ol[None, :]) @ wl
        absum = ((np.abs(xl) + np.abs(ol)[None, :]) @ np.abs(wl)).astype(np.float64)
    return ref, (n_cols + 2) * UL * absum, absum


def project_bound(n_cols, absum, dtype):
    """gamma_{n4+4} * absum + n4 * tiny in the compute type `dtype` (the module's docstring derives it)."""
    sz = np.dtype(dtype).itemsize
    n4 = -(-int(n_cols) // 4) * 4
    return gamma(n4 + 4, UNIT[sz]) * np.asarray(absum, np.float64) + n4 * TINY[sz]


def assert_project_within(got, x, offset, weights, dtype):
    """got within project_bound + the reference's own error of the longdouble reference wherever that is finite; -> the largest
    error / allowance."""
    ref, ref_err, absum = project_reference(x, offset, weights)
    allow = project_bound(np.asarray(x).shape[1], absum, dtype) + ref_err
    fin = np.isfinite(ref.astype(np.float64)) & np.isfinite(absum)
    assert got.shape == ref.shape and got.dtype == np.dtype(dtype)
    assert np.isfinite(got[fin]).all()
    err = np.abs(got.astype(np.longdouble) - ref)[fin]
    worst = float((err / allow[fin]).max()) if fin.any() else 0.0
    assert worst <= 1.0, 'max err / allowance %.3g' % worst
    return worst


def assert_same_bits(got, want):
    """NaNs compare as NaN, everything else by its bits, the sign of zero included."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    u = np.dtype('u%d' % got.dtype.itemsize)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), 'NaN pattern differs'
    same = (np.ascontiguousarray(got).view(u) == np.ascontiguousarray(want).view(u)) | nan
    if not same.all():
        at = tuple(int(v) for v in np.argwhere(~same)[0])
        raise AssertionError('%d of %d differ, first at %r: got %r want %r' % ((~same).sum(), same.size, at, got[at], want[at]))


class ProjectOracleCodec(LaneOracleCodec):
    """LaneOracleCodec + project restated in numpy: resident chunks read from the lane's cache dict (E_MISS when a chunk without
    bytes is not there), the others decoded and NOT inserted.  Records (lane, keys, lens, row_begin, row_end) of every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.project_calls = []

    def project(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, row_begin, row_end, cols, offset, weights,
                out_dtype, lane=None):
        dtype = np.dtype(dtype)
        self.project_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(row_begin), int(row_end)))
        cols = np.asarray(cols, dtype=np.int64)
        w = np.asarray(weights, dtype=np.float64)
        assert 1 <= cols.size <= 1024 and (cols >= 0).all() and (cols < n_channels).all()
        assert w.shape[0] == cols.size and 1 <= w.shape[1] <= 1024 and np.isfinite(w).all()
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        assert len(keys) and int(row0[0]) <= row_begin < row_end <= int(row0[-1]) + int(n_rows[-1]), 'chunks do not cover the rows'
        status, arrays = self._call_chunks('project', cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags, fill=True)
        x = np.concatenate(arrays, axis=0)[row_begin - int(row0[0]):row_end - int(row0[0])][:, cols]
        return status, project_chain(x, offset, w, out_dtype)
