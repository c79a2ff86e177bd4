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
        from mtscomp_amd import hip
        dtype = np.dtype(dtype)
        self.decimate_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens]))
        cache = self.caches.get(cache_id, {}) if cache_id else {}
        cols = np.asarray(cols, dtype=np.int64)
        assert q >= 1 and cols.size and (cols >= 0).all() and (cols < n_channels).all()
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        status, arrays = [], []
        for k, o, n, nr in zip(keys, offs, lens, n_rows):
            if not n:
                if k not in cache:
                    raise hip.HipError(hip.E_MISS, 'mts_decimate', 'chunk key %d is not resident' % k)
                status.append(0)
                arrays.append(cache[k])
                continue
            st, arrs = super(LaneOracleCodec, self).decompress([bytes(memoryview(cdata)[o:o + n])], [nr], n_channels, dtype, flags)
            self.calls.pop()
            status.append(st[0])
            arrays.append(arrs[0] if st[0] == 0 else np.zeros((nr, n_channels), dtype))
        x = np.concatenate(arrays, axis=0)[:, cols] if arrays else np.zeros((0, cols.size), dtype)
        y = fir_decimate(x, int(row0[0]) if len(keys) else 0, valid_begin, valid_end, first_row, n_out, q, taps, out_dtype)
        return status, y
