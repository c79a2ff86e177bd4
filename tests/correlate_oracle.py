"""Test-only restatements of mts_correlate in numpy: the definition of include/mtscomp_hip.h twice -- vectorised (on the filter and
the median of tests/detect_oracle.py and the exact fmaf of tests/project_oracle.py, one fmaf of whole (rows, templates) arrays per
(column, tau)) and by brute force (every score its own scalar chain, with libm's fmaf where it can be loaded) -- and a lane codec
built on the first so that the CPU suite drives Reader.correlate (argument handling, calls, lanes, cache use, errors) and can check
bit-identity."""
import ctypes
import ctypes.util

import numpy as np

from tests.codec_oracle import LaneOracleCodec
from tests.detect_oracle import filtered, row_median
from tests.project_oracle import fmaf_f32

NAN_BITS = 0x7fc00000
FILL = np.frombuffer(np.uint32(NAN_BITS).tobytes(), np.float32)[0]


def reference_rows(x, x_row0, vb, ve, a, b, taps, reference):
    """z (float32) for file rows [a, b): detect's z inside the recording [vb, ve), +0 outside."""
    n_cols = x.shape[1]
    z = np.zeros((max(b - a, 0), n_cols), np.float32)
    lo, hi = max(a, vb), min(b, ve)
    if lo < hi:
        y = filtered(x, x_row0, vb, ve, lo, hi, np.asarray(taps, dtype=np.float64))
        if reference:
            with np.errstate(invalid='ignore', over='ignore'):
                y = (y - row_median(y)[:, None]).astype(np.float32)
        z[lo - a:hi - a] = y
    return z


def _templates(templates, n_cols):
    """(K, T, n4) float32: rounded once, the columns padded with +0 to a multiple of 4."""
    with np.errstate(over='ignore'):
        k = np.asarray(templates).astype(np.float32)
    assert k.ndim == 3 and k.shape[2] == n_cols
    n4 = -(-n_cols // 4) * 4
    return np.concatenate([k, np.zeros(k.shape[:2] + (n4 - n_cols,), np.float32)], axis=2)


def correlate_chain(z, templates):
    """The chain on z (n + T - 1, n_cols) float32, row i of the result laid with template row 0 on z row i: acc = +0; for g in 0, 4,
    .. < n4: for tau < T: for j in g .. g + 3: acc = fmaf(z[i + tau, j], K[k, tau, j], acc); a NaN gets the bits 0x7fc00000."""
    z = np.asarray(z, np.float32)
    k = _templates(templates, z.shape[1])
    n_out, T, n4 = k.shape
    n = z.shape[0] - T + 1
    z = np.concatenate([z, np.zeros((z.shape[0], n4 - z.shape[1]), np.float32)], axis=1)
    acc = np.zeros((max(n, 0), n_out), np.float32)
    if n <= 0:
        return acc
    for g in range(0, n4, 4):
        for tau in range(T):
            for j in range(g, g + 4):
                acc = fmaf_f32(z[tau:tau + n, j:j + 1], k[None, :, tau, j], acc)
    acc[np.isnan(acc)] = FILL
    return acc


def correlate(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates):
    """score (i1 - i0, K) float32 for file rows [i0, i1).  x: the selected columns of file rows [x_row0, x_row0 + len(x)), any item
    type; [vb, ve): the recording; reference 0 / 1; templates (K, T, n_cols), template row `before` on the scored row."""
    T = np.asarray(templates).shape[1]
    z = reference_rows(x, x_row0, vb, ve, i0 - before, i1 - before + T - 1, taps, reference)
    return correlate_chain(z, templates)


# ---- the same definition by brute force: a scalar chain per (t, k) ---------------------------------------------------------------
def _libm_fmaf():
    for name in (ctypes.util.find_library('m'), 'libm.so.6'):
        try:
            f = ctypes.CDLL(name).fmaf
        except (OSError, AttributeError, TypeError):
            continue
        f.argtypes = [ctypes.c_float] * 3
        f.restype = ctypes.c_float
        return lambda a, b, c: np.float32(f(float(a), float(b), float(c)))
    return lambda a, b, c: fmaf_f32(np.float32(a), np.float32(b), np.float32(c))[()]


def correlate_brute(x, x_row0, vb, ve, i0, i1, taps, reference, before, templates):
    fmaf = _libm_fmaf()
    n_cols = x.shape[1]
    with np.errstate(over='ignore'):
        k = np.asarray(templates).astype(np.float32)
    n_out, T, _ = k.shape
    n4 = -(-n_cols // 4) * 4
    out = np.zeros((i1 - i0, n_out), np.float32)
    zero = np.float32(0.0)
    for t in range(i0, i1):
        a, b = max(vb, t - before), min(ve, t - before + T)
        z = reference_rows(x, x_row0, vb, ve, a, b, taps, reference) if a < b else None
        for o in range(n_out):
            acc = zero
            for g in range(0, n4, 4):
                for tau in range(T):
                    r = t - before + tau
                    for j in range(g, g + 4):
                        inside = vb <= r < ve and j < n_cols
                        acc = fmaf(z[r - a, j] if inside else zero, k[o, tau, j] if j < n_cols else zero, acc)
            out[t - i0, o] = FILL if np.isnan(acc) else acc
    return out


class CorrelateOracleCodec(LaneOracleCodec):
    """LaneOracleCodec + correlate restated in numpy: resident chunks read from the lane's cache dict (E_MISS when a chunk without
    bytes is not there), the others decoded and NOT inserted.  Records (lane, keys, lens, row_begin, row_end) of every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.correlate_calls = []
        self.miss_next_correlate = False             # simulate an entry dropped between the query and the call

    def correlate(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end,
                  taps, cols, reference, before, templates, lane=None):
        self.correlate_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(row_begin), int(row_end)))
        cols = np.asarray(cols, dtype=np.int64)
        taps = np.asarray(taps, dtype=np.float64)
        k = np.asarray(templates)
        assert 1 <= cols.size <= 1024 and (cols >= 0).all() and (cols < n_channels).all() and reference in (0, 1)
        assert k.ndim == 3 and k.dtype == np.float32 and k.shape[2] == cols.size and 1 <= k.shape[0] <= 1024 and 1 <= k.shape[1] <= 256
        assert np.isfinite(k).all() and 0 <= before <= k.shape[1]
        assert valid_begin <= row_begin < row_end <= valid_end
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        half = (taps.size - 1) // 2
        lo = max(valid_begin, row_begin - before + half - (taps.size - 1))
        hi = min(valid_end, row_end + k.shape[1] - before - 1 + half)
        assert lo < hi and int(row0[0]) <= lo and hi <= int(row0[-1]) + int(n_rows[-1]), 'the chunks do not cover the rows read'
        status, arrays = self._call_chunks('correlate', cache_id, keys, cdata, offs, lens, n_rows, n_channels, np.dtype(dtype), flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        return status, correlate(x, int(row0[0]), valid_begin, valid_end, row_begin, row_end, taps, reference, before, k)
