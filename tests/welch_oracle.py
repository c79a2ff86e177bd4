"""Test-only restatements of mts_welch in numpy: the summation tree of Reader.welch (blocks of B segments in order, groups of G
segments in block order, all float64), a lane codec built on it so that the CPU suite drives Reader.welch (argument handling, calls,
lanes, cache use, errors) and can check bit-identity, a float64 reference and the error bounds the GPU results are held to (uniform and
per bin), the kernel's plan and transform restated (welch_plan, kernel_rfft), and the deterministic edge cases both the CPU tests of
these references and the GPU tests run."""
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
        cols = np.asarray(cols, dtype=np.int64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all()
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        status, arrays = self._call_chunks('welch', cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags, fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        return status, welch_partials(x, int(row0[0]), row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend, compute_dtype)


# ---- the float64 reference and the bound -------------------------------------------------------------------------------------------
def welch_f64(x, start, stop, nperseg, step, taper, detrend, compute_dtype=None):
    """Reader.welch restated in float64 before scaling: (sum over segments of |X_k|^2 (nperseg // 2 + 1, n_cols), sum over segments of
    E = sum_n (w_n (x_n - m))^2 per column (n_cols,), n_seg, first).  x: the columns of the whole recording; the detrended values are
    formed as the kernel forms them (segment_mean), the FFT is numpy's in float64.  first: the first term of welch_bound_bins for
    the compute type, sum over segments of 2 |X_k| e + e^2 with e = delta sqrt(N E) of the segment and column, shaped like the sums
    (None when no compute type is given)."""
    n_seg = (stop - start - nperseg) // step + 1
    w = np.asarray(taper, np.float64)[:, None]
    tot = np.zeros((nperseg // 2 + 1, x.shape[1]))
    energy = np.zeros(x.shape[1])
    delta = None if compute_dtype is None else welch_delta(nperseg, compute_dtype)
    first = None if compute_dtype is None else np.zeros_like(tot)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(n_seg):
            r = start + k * step
            y = detrended(x[r:r + nperseg], detrend) * w
            X = np.fft.rfft(y, axis=0)
            p = X.real * X.real + X.imag * X.imag
            e_seg = (y * y).sum(axis=0)
            tot += p
            energy += e_seg
            if first is not None:
                e = delta * np.sqrt(nperseg * e_seg)[None, :]
                first += 2 * np.sqrt(p) * e + e * e
    return tot, energy, n_seg, first


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


def welch_delta(nperseg, compute_dtype):
    """delta = (c log2 N + 3) u_F + (c log2 N + 3) u64: kernel in F, reference in float64."""
    u = np.finfo(np.dtype(compute_dtype)).eps / 2
    u64 = np.finfo(np.float64).eps / 2
    lg = np.log2(nperseg)
    return (FFT_LEVEL_C * lg + 3) * u + (FFT_LEVEL_C * lg + 3) * u64


def welch_bound(nperseg, compute_dtype, energy, n_seg):
    """Per column: the largest |got - want| of the unscaled sums of |X_k|^2 (want = welch_f64's), every bin: (2 delta + delta^2) N
    sum_k E_k with delta = (c log2 N + 3) u + (c log2 N + 3) u64 (kernel in F, reference in float64), plus the float64 additions
    over segments, blocks and groups on both sides, 2 (n_seg + 2) u64 (1 + delta)^2 N sum_k E_k.  The same for every bin, so it
    is loose wherever a bin holds less than the segment's whole energy: the tests use welch_bound_bins, which is never larger."""
    u64 = np.finfo(np.float64).eps / 2
    delta = welch_delta(nperseg, compute_dtype)
    ne = nperseg * np.asarray(energy, np.float64)
    return (2 * delta + delta * delta) * ne + 2 * (n_seg + 2) * u64 * (1 + delta) ** 2 * ne


# The bound per bin.  delta is kept as derived above; only the step "|X_f| <= sqrt(N E)" is not taken.  For segment s, column j, bin k
# write X for the exact spectrum of y, X^ for the kernel's (in F) and X~ for the reference's (numpy, float64).
#   1. A 2-norm bound holds for each component: |X^_k - X_k| <= ||X^ - X||_2 <= delta_F sqrt(N E_s), likewise |X~_k - X_k| <= delta_64
#      sqrt(N E_s) (the derivation above; ||X||_2^2 = N E_s by Parseval).  Triangle inequality: |X^_k - X~_k| <= delta sqrt(N E_s)
#      =: e_s with delta = delta_F + delta_64.  (E_s as summed in float64 is off by a few u64 relative; c = 10 >= 9.4 covers that.)
#   2. | |X^_k|^2 - |X~_k|^2 | = | |X^_k| - |X~_k| | (|X^_k| + |X~_k|) <= e_s (2 |X~_k| + e_s) = 2 |X~_k| e_s + e_s^2: the reverse
#      triangle inequality, then |X^_k| <= |X~_k| + e_s.  It is stated on the reference's own |X~_k|, which welch_f64 has in hand.
#   3. Summed over the segments: first_k = sum_s (2 |X~_{k,s}| e_s + e_s^2)      (welch_f64's fourth result).
#   4. The float64 work after the transform.  Each side squares and adds two components (relative error <= 2 u64 on a sum of two
#      non-negative products) and adds n_seg non-negative terms in some order, n_seg - 1 additions whatever the tree of blocks,
#      groups and calls (Higham, sec. 4.2: relative error <= (n - 1) u64 + O(u64^2) for non-negative terms, any order): each
#      side's sum is within (n_seg + 2) u64 of its exact sum, one u64 of that left for the second-order terms (n_seg u64 << 1).  The
#      reference's exact sum is tot_k, the kernel's at most tot_k + first_k (step 3), so the term is 2 (n_seg + 2) u64 (tot_k +
#      first_k), per bin -- not relative to N sum E.
# With |X~_k| <= sqrt(N E_s) (Cauchy-Schwarz) first_k <= (2 delta + delta^2) N sum E and tot_k + first_k <= (1 + delta)^2 N sum E:
# welch_bound_bins <= welch_bound in every bin, with equality only where one bin holds the whole energy (a constant column's bin 0
# without detrend), there up to the rounding of the two expressions.  No constant here comes from a measurement.
# A tighter e_s = eta ||y_s||_1 (a componentwise bound through the butterfly matrices) is not used: the split step mixes Z_k and
# Z_{M-k} with a twiddle, and its componentwise constant was not derived; nothing is fitted in its place.
def welch_bound_bins(tot, first, n_seg):
    """Per bin and column: the largest |got - want| of the unscaled sums of |X_k|^2, want = tot and first = welch_f64's for the
    compute type: first + 2 (n_seg + 2) u64 (tot + first)."""
    u64 = np.finfo(np.float64).eps / 2
    tot, first = np.asarray(tot, np.float64), np.asarray(first, np.float64)
    return first + 2 * (n_seg + 2) * u64 * (tot + first)


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


# ---- the kernel's plan, restated ---------------------------------------------------------------------------------------------------
WT = 512                                                                 # threads per workgroup
TILE_BYTES = 65536                                                       # LDS for a tile's points


def welch_plan(compute_dtype, nperseg):
    """WPlan<F, log2 nperseg> of welch.hip: C columns per tile, P threads per column, K contiguous rows per thread and segment, BINS
    bins per thread (thread p of a column holds bins p + P i, i < BINS; p = 0 also bin N / 2; rows p K .. p K + K - 1; rows n, n + 1
    (n even) are the real and imaginary part of point n / 2), lds: the tile's bytes."""
    size = np.dtype(compute_dtype).itemsize
    c0 = TILE_BYTES // (nperseg * size)
    C = 1 if c0 < 1 else 64 if c0 > 64 else c0
    P = WT // C
    return dict(C=C, P=P, K=nperseg // P, BINS=(nperseg // 2) * C // WT, lds=C * nperseg * size)


# ---- structured inputs: bins far below the segment's energy -----------------------------------------------------------------------
SHARE_F64 = 0.9


def structured_signals(nperseg, seed=0):
    """{name: (x (rows, n_cols) of one item type, {detrend: share})}: 5 nperseg + 7 rows (8 segments at half overlap from row 3,
    Hann).  share: per column, the least share of bins whose per-bin float32 bound is below the bin's power -- the smallest over
    nperseg 16 .. 16384 of what welch_f64 gives for these very arrays (computed on the CPU, figures beside each), rounded down; in
    float64 every share is 1 and SHARE_F64 is asked."""
    N = nperseg
    rows = 5 * N + 7
    rs = np.random.RandomState([seed, N])
    n = np.arange(rows, dtype=np.float64)
    ph = 2 * np.pi * n / N
    tones = np.stack([
        3000 * np.sin(ph * (N // 4)) + 30 * rs.randn(rows),              # a tone on a bin, noise 40 dB below            (1.0)
        3000 * np.sin(ph * (N // 8 + 0.5)) + 30 * rs.randn(rows),        # a tone between two bins                       (1.0)
        20000 * np.sin(ph * (N // 8)) + 20 * np.sin(ph * (3 * N // 8) + 1.0) + 30 * rs.randn(rows),   # two tones 60 dB apart (0.167)
        8000 * np.sin(np.pi * n * n / (4 * rows)),                        # a chirp, 0 to a quarter of the rate           (0.5)
    ], axis=1)
    walk = np.cumsum(rs.randn(rows, 2) * 100, axis=0)                     # 1 / f^2-like: most power in the lowest bins
    off = rs.randn(rows, 2)
    return {
        'tones_int16': (np.rint(tones).astype(np.int16), {True: (0.9, 0.9, 0.1, 0.4)}),
        'walk_int32': (np.rint(walk).astype(np.int32), {True: (0.9, 0.9), False: (0.3, 0.3)}),             # (1.0; 0.525, 0.403)
        'offset_uint16': (np.rint(30000 + 200 * off).astype(np.uint16), {True: (0.9, 0.9), False: (0.9, 0.9)}),   # (1.0)
        'offset_int64': ((1 << 62) + np.rint((1 << 55) * off).astype(np.int64), {True: (0.9, 0.9), False: (0.9, 0.9)}),   # (1.0)
        'offset_float32': ((1e6 + 5000 * off).astype(np.float32), {True: (0.9, 0.9), False: (0.9, 0.9)}),  # (1.0)
    }


def plan_rows(nperseg):
    """Rows of a segment chosen from both plans (float32 and float64): of threads p = 0, P // 2 and P - 1 the first row, its pair
    partner (an even and an odd row: y.x and y.y of one point) and the last of the K rows."""
    rows = set()
    for cdt in (np.float32, np.float64):
        pl = welch_plan(cdt, nperseg)
        for p in (0, pl['P'] // 2, pl['P'] - 1):
            rows.update((p * pl['K'], p * pl['K'] + 1, p * pl['K'] + pl['K'] - 1))
    return sorted(rows)


def sparse_case(nperseg):
    """Impulses in single segments, a column per pattern.  -> (x int16 (rows, n_cols), chunk_rows, starts, patterns).  Chunks are
    2 nperseg rows long; segment i (i = 1, 2, 3) starts at starts[i - 1] = i chunk_rows - b_i so that the chunk boundary falls at
    its row b_i: inside a thread's K rows (b_1 = p K + 2, or p K + 1 where K = 2), between two threads (b_2 = p K) and between the two
    rows of a pair (b_3 = p K + 1), p = P // 2 of the float32 plan.  patterns[j]: the rows of column j's impulses within every
    segment (one row or two): plan_rows and the rows on both sides of each boundary; pairs join neighbours of that list."""
    N = nperseg
    pl = welch_plan(np.float32, N)
    pk = (pl['P'] // 2) * pl['K']
    bs = [pk + (2 if pl['K'] > 2 else 1), pk, pk + 1]
    L = 2 * N
    starts = [(i + 1) * L - b for i, b in enumerate(bs)]
    rows = sorted(set(plan_rows(N)) | {b - 1 for b in bs} | set(bs))
    patterns = [(r,) for r in rows] + [(rows[i], rows[(i + 1) % len(rows)]) for i in range(len(rows))] + [(rows[0], rows[len(rows) // 2])]
    x = np.zeros((4 * L + 3, len(patterns)), np.int16)
    for j, pat in enumerate(patterns):
        for s0 in starts:
            for q, r in enumerate(pat):
                x[s0 + r, j] = (1000, -700)[q] + 13 * j
    return x, L, starts, patterns


def block_case(compute_dtype, nperseg, n_seg=70, seed=0):
    """More than two blocks of segments, not a multiple of B, on a tile and one column more.  -> (x int16 (n_seg nperseg, C),
    channels (C + 1, one of them a repeat)).  Segment s (noverlap 0) holds one impulse of its own amplitude 1000 + 14 s + column at
    a row of its own, so that with a boxcar every bin of segment s holds amplitude^2."""
    C = welch_plan(compute_dtype, nperseg)['C']
    rs = np.random.RandomState([seed, nperseg, C])
    x = np.zeros((n_seg * nperseg, C), np.int16)
    for j in range(C):
        x[np.arange(n_seg) * nperseg + rs.randint(0, nperseg, size=n_seg), j] = 1000 + 14 * np.arange(n_seg) + j
    return x, [int(c) for c in rs.permutation(C)] + [int(rs.randint(C))]


def array_tapers(nperseg):
    """Two tapers without symmetry: pseudo-random in [0.1, 1.1], and the same with alternating signs."""
    w = np.random.RandomState([7, nperseg]).rand(nperseg) + 0.1
    return w, w * np.where(np.arange(nperseg) & 1, -1.0, 1.0)


# ---- the kernel's transform, restated in the compute type -------------------------------------------------------------------------
def twiddles(nperseg, compute_dtype):
    """tw[q] = exp(-2 pi i q / N), q < N, as (re, im): from numpy's widest float (the library: long double), rounded once to F."""
    a = 2 * np.pi * np.arange(nperseg, dtype=np.longdouble) / nperseg
    F = np.dtype(compute_dtype)
    return np.cos(a).astype(F), (-np.sin(a)).astype(F)


def kernel_rfft(y, compute_dtype, mutant=None):
    """The N / 2 + 1 bins of the real FFT of y (N, n_cols), every operation in F, by k_welch's steps and index arithmetic: rows n,
    n + 1 packed as point n / 2, Stockham passes of radix 4 (and one of radix 2 when log2(N / 2) is odd) with j, k, sh and d0 as in
    fft_pass, the split with tw[k], bins 0 and N / 2 from Z[0].  -> (re, im) in F.  mutant 'split_tw': the split of bin k = N / 4 + 1
    takes tw[k + 1]."""
    F = np.dtype(compute_dtype)
    N = y.shape[0]
    M, lg = N // 2, int(np.log2(N))
    twr, twi = twiddles(N, F)
    zr, zi = y[0::2].astype(F), y[1::2].astype(F)

    def cmul(ar, ai, wr, wi):
        return ar * wr - ai * wi, ar * wi + ai * wr

    lns = 0
    while lns < lg - 1:
        R, LR = (4, 2) if lns + 2 <= lg - 1 else (2, 1)
        j = np.arange(M // R)
        k = j & ((1 << lns) - 1)
        vr = [zr[j + r * (M // R)] for r in range(R)]
        vi = [zi[j + r * (M // R)] for r in range(R)]
        if lns > 0:
            sh = lg - lns - LR
            for r in range(1, R):
                q = (k * r) << sh
                vr[r], vi[r] = cmul(vr[r], vi[r], twr[q][:, None], twi[q][:, None])
        if R == 4:
            ar, ai, br, bi = vr[0] + vr[2], vi[0] + vi[2], vr[0] - vr[2], vi[0] - vi[2]
            cr, ci, dr, di = vr[1] + vr[3], vi[1] + vi[3], vr[1] - vr[3], vi[1] - vi[3]
            outr = [ar + cr, br + di, ar - cr, br - di]
            outi = [ai + ci, bi - dr, ai - ci, bi + dr]
        else:
            outr = [vr[0] + vr[1], vr[0] - vr[1]]
            outi = [vi[0] + vi[1], vi[0] - vi[1]]
        d0 = ((j >> lns) << (lns + LR)) + k
        zr, zi = np.empty_like(zr), np.empty_like(zi)
        for r in range(R):
            zr[d0 + (r << lns)] = outr[r]
            zi[d0 + (r << lns)] = outi[r]
        lns += LR
    xr, xi = np.zeros((M + 1,) + y.shape[1:], F), np.zeros((M + 1,) + y.shape[1:], F)
    xr[0], xr[M] = zr[0] + zi[0], zr[0] - zi[0]
    k = np.arange(1, M)
    half = F.type(0.5)
    ar, ai, br, bi = zr[k], zi[k], zr[M - k], zi[M - k]
    er, ei, o_r, oi = (ar + br) * half, (ai - bi) * half, (ai + bi) * half, (br - ar) * half
    q = k.copy()
    if mutant == 'split_tw':
        q[M // 2] += 1                                                   # (k = M / 2 + 1 takes tw[k + 1])
    wr, wi = twr[q][:, None], twi[q][:, None]
    xr[1:M] = er + (wr * o_r - wi * oi)
    xi[1:M] = ei + (wr * oi + wi * o_r)
    return xr, xi


def kernel_welch(x, start, stop, nperseg, step, taper, detrend, compute_dtype, mutant=None):
    """Reader.welch's unscaled sums by kernel_rfft: y = F(double(x) - m) F(taper), P = double(re)^2 + double(im)^2, added in float64
    in segment order.  mutant: None, 'split_tw' (kernel_rfft), 'taper' (taper[n ^ 1]), 'row' (row N / 2 + 1 of every segment reads
    row N / 2's item), 'seg31' (the last segment of every full block of B is not added), 'mean32' (the mean rounded to float32)."""
    F = np.dtype(compute_dtype)
    N = nperseg
    n_seg = (stop - start - N) // step + 1
    w = np.asarray(taper, np.float64).astype(F)
    if mutant == 'taper':
        w = w[np.arange(N) ^ 1]
    tot = np.zeros((N // 2 + 1, x.shape[1]))
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(n_seg):
            if mutant == 'seg31' and s % B == B - 1:
                continue
            seg = x[start + s * step:start + s * step + N]
            m = segment_mean(seg) if detrend else 0.0
            if mutant == 'mean32':
                m = np.float64(np.float32(m))
            d = seg.astype(np.float64) - m
            if mutant == 'row':
                d[N // 2 + 1] = d[N // 2]
            re, im = kernel_rfft(d.astype(F) * w[:, None], F, mutant)
            re, im = re.astype(np.float64), im.astype(np.float64)
            tot = tot + (re * re + im * im)
    return tot


# ---- the deterministic edge cases, shared by the CPU tests of the references and the GPU tests -----------------------------------
def bins_case(nperseg):
    """Columns whose power sits in one bin with a boxcar and no detrend: x[n] = 1500 (-1)^n (bin N / 2), x[n] = -1234 (bin 0),
    x[n] = 77 (-1)^n + 5 (both); 4 nperseg rows, noverlap 0 from row 0 (an even row: the sign of (-1)^n is the segment's)."""
    n = np.arange(4 * nperseg)
    alt = np.where(n & 1, -1, 1)
    return np.stack([1500 * alt, np.full(n.size, -1234), 77 * alt + 5], axis=1).astype(np.int16)


def edge_cases(nperseg):
    """[(name, x, [(start, stop, noverlap, window, detrend), ...], shares or None)]: the structured spectra, the sparse segments and the
    one-bin columns at this nperseg; shares: per detrend and column, the least share of bins with float32 bound < power."""
    N = nperseg
    out = []
    for name, (x, shares) in structured_signals(N).items():
        out.append((name, x, [(3, x.shape[0], N // 2, 'hann', d) for d in shares], shares))
    x, _, starts, _ = sparse_case(N)
    w_pos, w_alt = array_tapers(N)
    out.append(('sparse', x, [(s0, s0 + N, 0, w, False) for s0 in starts for w in ('boxcar', w_pos, w_alt)], None))
    out.append(('one_bin', bins_case(N), [(0, 4 * N, 0, 'hann', False), (0, 4 * N, N // 2, 'hann', True)], None))
    return out
