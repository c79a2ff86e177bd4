"""Test-only restatements of mts_welch in numpy: the summation tree of Reader.welch (blocks of B segments in order, groups of G
segments in block order, all float64), a lane codec built on it so that the CPU suite drives Reader.welch (argument handling, calls,
lanes, cache use, errors) and can check bit-identity, a float64 reference and the error bound the GPU results are held to."""
import numpy as np

from mtscomp_amd import hip
from tests.codec_oracle import LaneOracleCodec

B = hip.WELCH_BLOCK_SEGMENTS


def segment_mean(seg):
    """The mean of each column of a segment (nperseg rows, nperseg a power of two), as the kernel forms it: integers -- the exact
    sum rounded once to float64, divided by nperseg; floats -- the pairwise tree v = v[0::2] + v[1::2] in float64, divided."""
    n = seg.shape[0]
    if seg.dtype.kind in 'iu':
        if seg.dtype.itemsize < 8:
            s = seg.astype(np.int64).sum(axis=0)
            return s.astype(np.float64) / n
        s = seg.astype(object).sum(axis=0)
        return np.array([float(int(v)) for v in s], dtype=np.float64).reshape(seg.shape[1:]) / n
    v = seg.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        while v.shape[0] > 1:
            v = v[0::2] + v[1::2]
    return v[0] / n


def detrended(seg, detrend):
    """double(x) - mean (or double(x)), float64."""
    with np.errstate(invalid='ignore', over='ignore'):
        x = seg.astype(np.float64)
        return x - segment_mean(seg) if detrend else x


def segment_power(seg, taper, detrend, compute_dtype):
    """|X_k|^2 in float64 of one segment (nperseg, n_cols): y = F(x - m) * F(taper) in F, X = rfft(y) in F."""
    F = np.dtype(compute_dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        y = detrended(seg, detrend).astype(F) * np.asarray(taper, np.float64).astype(F)[:, None]
        X = np.fft.rfft(y, axis=0)
        re, im = X.real.astype(np.float64), X.imag.astype(np.float64)
        return re * re + im * im


def welch_partials(x, x_row0, row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend, compute_dtype):
    """The group sums mts_welch returns for segments [seg_begin, seg_end) (seg_begin a multiple of G), x: 2-D items holding file
    rows [x_row0, x_row0 + len(x)).  -> (n_groups, nperseg // 2 + 1, n_cols) float64."""
    G = hip.welch_group_segments(step)
    assert seg_begin % G == 0
    n_groups = -(-(seg_end - seg_begin) // G)
    out = np.zeros((n_groups, nperseg // 2 + 1, x.shape[1]))
    for g in range(n_groups):
        acc = np.zeros(out.shape[1:])
        for b0 in range(seg_begin + g * G, min(seg_begin + (g + 1) * G, seg_end), B):
            blk = None
            for s in range(b0, min(b0 + B, seg_end)):
                r = row_seg0 + s * step - x_row0
                assert 0 <= r and r + nperseg <= x.shape[0], 'rows outside the chunks given'
                p = segment_power(x[r:r + nperseg], taper, detrend, compute_dtype)
                with np.errstate(invalid='ignore', over='ignore'):
                    blk = p if blk is None else blk + p
            with np.errstate(invalid='ignore', over='ignore'):
                acc = acc + blk
        out[g] = acc
    return out


class WelchOracleCodec(LaneOracleCodec):
    """LaneOracleCodec + welch restated in numpy: resident chunks read from the lane's cache dict (E_MISS when a chunk without bytes
    is not there), the others decoded and NOT inserted.  Records (lane, keys, lens, seg_begin, seg_end) of every call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.welch_calls = []

    def welch(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, row_seg0, seg_begin, seg_end, nperseg, step,
              taper, detrend, compute_dtype, cols, lane=None):
        dtype = np.dtype(dtype)
        self.welch_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(seg_begin), int(seg_end)))
        cache = self.caches.get(cache_id, {}) if cache_id else {}
        cols = np.asarray(cols, dtype=np.int64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all()
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        status, arrays = [], []
        for k, o, n, nr in zip(keys, offs, lens, n_rows):
            if not n:
                if k not in cache:
                    raise hip.HipError(hip.E_MISS, 'mts_welch', 'chunk key %d is not resident' % k)
                status.append(0)
                arrays.append(cache[k])
                continue
            st, arrs = super(LaneOracleCodec, self).decompress([bytes(memoryview(cdata)[o:o + n])], [nr], n_channels, dtype, flags)
            self.calls.pop()
            status.append(st[0])
            arrays.append(arrs[0] if st[0] == 0 else np.zeros((nr, n_channels), dtype))
        x = np.concatenate(arrays, axis=0)[:, cols]
        return status, welch_partials(x, int(row0[0]), row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend, compute_dtype)


# ---- the float64 reference and the bound -------------------------------------------------------------------------------------------
def welch_f64(x, start, stop, nperseg, step, taper, detrend):
    """Reader.welch restated in float64 before scaling: (sum over segments of |X_k|^2 (nperseg // 2 + 1, n_cols), sum over segments of
    E = sum_n (w_n (x_n - m))^2 per column (n_cols,), n_seg).  x: the columns of the whole recording; the detrended values are
    formed as the kernel forms them (segment_mean), the FFT is numpy's in float64."""
    n_seg = (stop - start - nperseg) // step + 1
    w = np.asarray(taper, np.float64)[:, None]
    tot = np.zeros((nperseg // 2 + 1, x.shape[1]))
    energy = np.zeros(x.shape[1])
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(n_seg):
            r = start + k * step
            y = detrended(x[r:r + nperseg], detrend) * w
            X = np.fft.rfft(y, axis=0)
            tot += X.real * X.real + X.imag * X.imag
            energy += (y * y).sum(axis=0)
    return tot, energy, n_seg


# c: the relative 2-norm error an FFT level adds.  Higham, Accuracy and Stability of Numerical Algorithms (2nd ed.), Thm 24.2: a
# radix-2 level with twiddles of error mu costs eta = mu + gamma_4 (sqrt(2) + mu) <= (1 + 4 sqrt(2)) u + O(u^2) ~ 6.66 u with
# mu <= u (a twiddle rounded once from extended precision; a radix-4 pass is two radix-2 levels whose inner twiddles, +-1 and +-i,
# are exact).  The N / 2-point complex FFT has log2(N) - 1 levels; the split X_k = (Z_k + conj Z_{M-k}) / 2 + W^k (Z_k - conj Z_{M-k})
# / 2i has norm <= 2 on Z, so it carries the complex FFT's error times 2 ||Z|| / ||X|| = sqrt(2), and adds one more level of rounding
# (two additions, an exact halving, a complex multiply and an addition: below the 6.66 u * sqrt(2) of a level).  Hence per segment
# ||X^ - X||_2 <= (sqrt(2) * 6.66 u * log2(N) + 3 u) ||X||_2 with 9.4 <= c = 10; the 3 u are x - m rounded to F, the taper rounded
# to F and their product.  ||X||_2^2 = N E (Parseval, over all N bins), so |X^_f| - |X_f| <= delta sqrt(N E), |X_f| <= sqrt(N E) and
# ||X^_f|^2 - |X_f|^2| <= (2 delta + delta^2) N E per segment.  The reference has its own float64 FFT error of the same form in u64.
FFT_LEVEL_C = 10


def welch_bound(nperseg, compute_dtype, energy, n_seg):
    """Per column: the largest |got - want| of the unscaled sums of |X_k|^2 (want = welch_f64's), every bin: (2 delta + delta^2) N
    sum_k E_k with delta = (c log2 N + 3) u + (c log2 N + 3) u64 (kernel in F, reference in float64), plus the float64 additions
    over segments, blocks and groups on both sides, 2 (n_seg + 2) u64 (1 + delta)^2 N sum_k E_k."""
    u = np.finfo(np.dtype(compute_dtype)).eps / 2
    u64 = np.finfo(np.float64).eps / 2
    lg = np.log2(nperseg)
    delta = (FFT_LEVEL_C * lg + 3) * u + (FFT_LEVEL_C * lg + 3) * u64
    ne = nperseg * np.asarray(energy, np.float64)
    return (2 * delta + delta * delta) * ne + 2 * (n_seg + 2) * u64 * (1 + delta) ** 2 * ne


def psd_scale(nperseg, taper, scaling, fs, n_seg):
    """What Reader.welch multiplies the sums by, per bin."""
    w = np.asarray(taper, np.float64)
    s = 1.0 / (fs * (w * w).sum()) if scaling == 'density' else 1.0 / w.sum() ** 2
    k = np.full(nperseg // 2 + 1, 2.0 * s / n_seg)
    k[0] = k[-1] = s / n_seg
    return k


def assert_welch_close(got, want, bound):
    """|got - want| <= bound where want and bound are finite; non-finite where want is not.  Returns the largest error / bound."""
    got = np.asarray(got, np.float64)
    want, bound = np.broadcast_arrays(np.asarray(want, np.float64), np.asarray(bound, np.float64))
    fin = np.isfinite(want) & np.isfinite(bound)
    assert not np.isfinite(got[~np.isfinite(want)]).any(), 'finite where the reference is not'
    err = np.abs(got[fin] - want[fin])
    assert np.isfinite(got[fin]).all(), 'non-finite where the reference is finite'
    b = bound[fin] + np.finfo(np.float64).tiny
    assert np.all(err <= b), float((err / b).max())
    return float((err / b).max()) if err.size else 0.0
