"""The cases of tests/test_gpu_detect_edges.py (k_row_median, k_detect_mask, k_detect_count / scan / emit and detect_run's slabs on the
MI355X) and of their CPU twins in tests/test_detect_oracles.py (the numpy stand-in DetectOracleCodec, and the brute-force restatement
at small shapes): the inputs and the checks are the same code, only the codec behind the Reader and the sizes differ.  Every
comparison is byte for byte against tests/detect_oracle.py over the oracle codec's decode; no tolerance anywhere.

make(x, chunk_rows) -> (Reader, the oracle's decode) is the caller's: the GPU file opens one lane on device 0, the twins the stand-in."""
import numpy as np

from mtscomp_amd import api, hip
from tests.cov_quantile_cases import recording  # noqa: F401  (the callers' make() is built on it)
from tests.detect_oracle import SIGNS, detect_events, detect_events_brute, filtered

TINY = float(np.finfo(np.float32).tiny)                        # 2^-126
SUBNORMAL = float(np.finfo(np.float32).smallest_subnormal)     # 2^-149
FMAX = float(np.finfo(np.float32).max)

# the geometry of detect.hip's compaction: a block of the bitmap is 1024 words (256 threads x 4), and the one workgroup of k_detect_scan
# gives each of its 256 threads ceil(blocks / 256) blocks
BLOCK_WORDS, SCAN_THREADS = 1024, 256


def scan_shape(rows, n_cols):
    """(bitmap words, blocks, blocks per thread of k_detect_scan) of a slab of `rows` rows x n_cols columns."""
    words = rows * ((n_cols + 63) // 64)
    blocks = -(-words // BLOCK_WORDS)
    return words, blocks, -(-blocks // SCAN_THREADS)


def want_events(dec, cols, threshold, start=0, stop=None, taps=None, sign='neg', reference=None, exclude=0, spread=0, brute=False):
    """The oracle's (row, pos, amp) of the call; brute: the brute-force restatement must agree."""
    n = dec.shape[0]
    args = (dec[:, cols], 0, 0, n, start, n if stop is None else stop, [1.0] if taps is None else taps, threshold, SIGNS[sign],
            1 if reference else 0, exclude, spread)
    want = detect_events(*args)
    if brute:
        other = detect_events_brute(*args)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(want, other)), 'the two restatements differ'
    return want


def check(r, dec, cols, threshold, start=0, stop=None, brute=False, **kw):
    """Reader.detect against the oracle, byte for byte.  -> (the Bunch, the oracle's arrays)."""
    cols = np.asarray(cols, dtype=np.int64)
    want = want_events(dec, cols, threshold, start, stop, brute=brute, **kw)
    got = r.detect(threshold, start, stop, channels=[int(c) for c in cols], **kw)
    assert got.sample.dtype == got.channel.dtype == np.int64 and got.amplitude.dtype == np.float32
    assert got.sample.tobytes() == want[0].tobytes(), ('sample', got.sample.size, want[0].size, got.sample[:6], want[0][:6])
    assert got.channel.tobytes() == cols[want[1]].tobytes(), 'channel'
    assert got.amplitude.tobytes() == want[2].tobytes(), 'amplitude'
    return got, want


def _dump(r, dec, cols, taps, reference, start=0, stop=None, threshold=TINY, brute=False):
    stop = dec.shape[0] if stop is None else stop
    _, want = check(r, dec, cols, threshold, start, stop, brute=brute, taps=taps, sign='both', reference=reference, exclude=0, spread=0)
    return want[0].size / float(max(1, (stop - start) * len(cols))), want


def dump(r, dec, cols, taps, reference, **kw):
    """detect as a dump of z: sign='both', no neighbours, the smallest normal float32 as the threshold -- every sample with |z| > 2^-126
    comes back with its amplitude, so byte equality checks the filter and the reference on every row, not the presence of a few events.
    -> the share of the samples the oracle emits."""
    return _dump(r, dec, cols, taps, reference, **kw)[0]


def pairs_of(got):
    return set(zip(got.sample.tolist(), got.channel.tolist()))


class Spy:
    """Around codec.detect: records every call's arguments and result, so that a test sees the buffer sizes the Reader chose, and can
    make the device call again with another max_events."""

    def __init__(self, monkeypatch, r):
        self.calls, self.orig = [], r.codec.detect
        monkeypatch.setattr(r.codec, 'detect', self)

    def __call__(self, *args, **kw):
        out = self.orig(*args, **kw)
        self.calls.append((args, kw, out))
        return out

    def caps(self):
        return [int(args[-1]) for args, _, _ in self.calls]

    def with_cap(self, i, cap):
        """Call i once more with max_events = cap.  -> (status, n_events, row, pos, amp)."""
        args, kw, _ = self.calls[i]
        return self.orig(*(args[:-1] + (int(cap),)), **kw)


def plain_env(monkeypatch):
    """The library reads these with getenv on every call: unset, one piece and one slab hold a small recording."""
    monkeypatch.delenv('MTS_PIPE_BYTES', raising=False)
    monkeypatch.delenv('MTS_DETECT_SLAB_BYTES', raising=False)


def slab_bytes(n_cols, own, R):
    """MTS_DETECT_SLAB_BYTES for which a slab owns `own` rows: the workspace holds them and R rows either side, float32."""
    return 4 * n_cols * (own + 2 * R)


# ---- 1. the median network at every size --------------------------------------------------------------------------------------------
MEDIAN_NS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
MEDIAN_RANDOM_ROWS = 40                                        # rows [0, 40): continuous random values, the rows of the share


def network_size(n):
    P = 2
    while P < n:
        P <<= 1
    return P


def median_recording(dtype, rows=200, nc=1024, ns=MEDIAN_NS):
    """Row families, one after the other (and once more from the start while rows remain): random; five distinct values; ascending;
    descending; constant; float32 only: a NaN at the first column, at column n // 2 and at column n - 1 of every n; +inf and -inf in one
    row; for every even n, the two middle values of the first n columns near FLT_MAX (either sign) -- the sum overflows, the median is
    +-inf, z is -+inf, or NaN where the row holds an inf as well --; rows of subnormals, whose median, mean of two and differences are
    subnormal."""
    dt = np.dtype(dtype)
    rs = np.random.RandomState(1024 + dt.itemsize)
    flt = dt.kind == 'f'
    x = (rs.randn(rows, nc) * 100).astype(dt) if flt else rs.randint(-32768, 32768, size=(rows, nc)).astype(dt)
    t = MEDIAN_RANDOM_ROWS

    def put(row):
        nonlocal t
        if t < rows:
            x[t] = row
            t += 1

    ramp = (np.arange(nc) - nc // 3).astype(dt)
    for _ in range(2):
        for k in range(6):
            put((rs.randint(-2, 3, nc) * 7).astype(dt))                       # five values
        put(ramp)
        put(ramp[::-1])
        put(np.sort(x[0]))
        put(np.sort(x[1])[::-1])
        put(np.full(nc, 5, dt))
        if not flt:
            continue
        for c in sorted({0} | {n // 2 for n in ns} | {n - 1 for n in ns}):     # one NaN: the median and every z of the row are NaN
            row = (rs.randn(nc) * 100).astype(dt)
            row[c] = np.nan
            put(row)
        row = (rs.randn(nc) * 100).astype(dt)
        row[[0, 1, nc // 2, nc - 1]] = [np.inf, -np.inf, np.inf, -np.inf]
        put(row)
        for n in ns:
            if n % 2 or n < 2:
                continue
            for sgn in (1.0, -1.0):
                row = (rs.randn(nc) * 100).astype(dt)                          # n / 2 - 1 values below, the two in the middle, the rest above
                row[n // 2 - 1:n // 2 + 1] = sgn * 0.9 * FMAX
                row[n // 2 + 1:n] = sgn * FMAX
                put(row)
            row = row.copy()
            if n >= 4:
                row[n - 1] = -np.inf                                           # (sgn = -1: the median is -inf, z of this column NaN)
                put(row)
        for k in range(4):
            put((rs.randint(-1000, 1001, nc) * SUBNORMAL).astype(dt))
        put((rs.randint(-2, 3, nc) * SUBNORMAL).astype(dt))                    # subnormal ties
    assert t > MEDIAN_RANDOM_ROWS + 20
    return x


def median_lists(n, nc, rs):
    """The first n columns in order, and n entries drawn from all of them: shuffled, with repeats."""
    return [np.arange(n), rs.randint(0, nc, n)]


def run_median(r, dec, ns=MEDIAN_NS, brute_upto=0):
    """Every list through the dump over the whole recording (the share: of its random rows) and through an ordinary call.
    -> {n: (share, events of the dump, events of the ordinary call, nonzero subnormal amplitudes)} of the in-order lists."""
    rows, nc = dec.shape
    flt = dec.dtype.kind == 'f'
    rs = np.random.RandomState(7)
    taps3 = [0.25, 0.5, 0.25]
    out = {}
    for n in ns:
        brute = n <= brute_upto
        for li, cols in enumerate(median_lists(n, nc, rs)):
            share_all, want = _dump(r, dec, cols, None, 'median', brute=brute)
            share = (want[0] < MEDIAN_RANDOM_ROWS).sum() / float(MEDIAN_RANDOM_ROWS * n)
            # an odd n has one z == 0 per row, its median: 1 - 1 / n of the samples at most; a repeated column can be the median twice
            if n >= 255 or (li == 0 and n % 2 == 0):
                assert share >= 0.99, (n, li, share)
            n_dump = want[0].size
            sure = n >= 63 or (li == 0 and n >= 2)                              # (two draws of one column: every z is 0)
            assert n_dump >= (rows * n // 4 if sure else 0), (n, li, n_dump)
            n_sub = 0
            if flt and li == 0:                     # the smallest threshold there is: the subnormal rows come back too
                _, want = check(r, dec, cols, SUBNORMAL, sign='both', reference='median')
                a = np.abs(want[2])
                n_sub = int(((a > 0) & (a < TINY)).sum())
                assert n_sub >= 1 or n < 2, n
                if n % 2 == 0:          # the overflowing middle: the median is +-inf, the amplitudes -+inf
                    assert np.isposinf(want[2]).any() and np.isneginf(want[2]).any(), n
            # an ordinary call: the scale from the oracle's own z of the random rows
            y = filtered(dec[:MEDIAN_RANDOM_ROWS][:, cols], 0, 0, MEDIAN_RANDOM_ROWS, 0, MEDIAN_RANDOM_ROWS, np.asarray(taps3)).astype(np.float64)
            z = y - np.median(y, axis=1)[:, None]
            thr = 1.5 * float(z.std()) if z.std() > 0 else 1.0
            got, _ = check(r, dec, cols, thr, 2, rows - 1, brute=brute, taps=taps3, sign='both', reference='median', exclude=3, spread=2)
            if li == 0:
                out[n] = (share, n_dump, got.sample.size, n_sub)
    assert sum(v[2] for v in out.values()) >= 50
    return out


# ---- 2. the scan beyond 256 blocks ---------------------------------------------------------------------------------------------------
def spiky_int8(rows, nc, n_spikes, seed):
    """int8 in [-100, 100] (1 in 201 is 0: the dump emits >= 0.99 of the samples) with n_spikes values of +-(110 .. 127)."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-100, 101, size=(rows, nc)).astype(np.int8)
    at = rs.randint(0, rows * nc, n_spikes)
    x.ravel()[at] = (rs.randint(110, 128, n_spikes) * rs.choice([-1, 1], n_spikes)).astype(np.int8)
    return x


def run_scan(r, dec, monkeypatch, caps=None, slab_own=None, brute=False):
    """Sparse (exclude 3, spikes only) and dense (the dump) over the whole range in one call; dense with the capacities `caps`
    (callables of the total); slab_own: MTS_DETECT_SLAB_BYTES so that a slab owns that many rows.  -> (sparse events, dense events)."""
    rows, nc = dec.shape
    cols = np.arange(nc)
    plain_env(monkeypatch)
    spy = Spy(monkeypatch, r)
    if slab_own:
        monkeypatch.setenv('MTS_DETECT_SLAB_BYTES', str(slab_bytes(nc, slab_own, 3)))
    _, want = check(r, dec, cols, 105.0, brute=brute, sign='both', exclude=3, spread=0)
    n_sparse = want[0].size
    if slab_own:
        monkeypatch.setenv('MTS_DETECT_SLAB_BYTES', str(slab_bytes(nc, slab_own, 0)))
    del spy.calls[:]
    share, want = _dump(r, dec, cols, None, None, brute=brute)
    assert share >= 0.99, share
    total = want[0].size
    # the Reader's own two calls: one part over the whole range, a first buffer too small, the second exact
    assert [(c[0][12], c[0][13]) for c in spy.calls] == [(0, rows)] * 2, [(c[0][12], c[0][13]) for c in spy.calls]
    assert spy.caps() == [max(api.DETECT_GUESS_MIN, rows * nc // api.DETECT_GUESS_SAMPLES), total] and spy.caps()[0] < total
    full = spy.calls[1][2]
    assert full[1] == total and full[2].size == total
    for cap in [c(total) for c in (caps or ())]:
        st, n_ev, row, pos, amp = spy.with_cap(0, cap)
        assert all(s == hip.CHUNK_OK for s in st) and n_ev == total and row.size == pos.size == amp.size == min(cap, total), cap
        assert (row.tobytes(), pos.tobytes(), amp.tobytes()) == (full[2][:cap].tobytes(), full[3][:cap].tobytes(), full[4][:cap].tobytes()), cap
    return n_sparse, total


SCAN_CAPS = (lambda total: total - 1, lambda total: 65536, lambda total: 65537, lambda total: 257, lambda total: 1, lambda total: 0)


# ---- 3. dense events and the second call -----------------------------------------------------------------------------------------------
def dense_masks(rows, nc):
    """Every sample; and a checkerboard with a diagonal on top, so that the popcounts of the words differ."""
    t, j = np.arange(rows)[:, None], np.arange(nc)[None, :]
    return [np.ones((rows, nc), bool), ((t + j) % 2 == 0) | (j % 7 == t % 5)]


def run_dense(r, mask, monkeypatch, n_chunks):
    """x = 7 where mask, else 0; threshold 1, no neighbours: exactly the samples of the mask, in (row, position) order, through a first
    buffer that is too small; then one call per chunk (DETECT_CALL_BYTES = 1), each made twice."""
    rows, nc = mask.shape
    plain_env(monkeypatch)
    ti, ji = np.nonzero(mask)
    spy = Spy(monkeypatch, r)
    for call_bytes, n_parts in ((api.DETECT_CALL_BYTES, 1), (1, n_chunks)):
        monkeypatch.setattr(api, 'DETECT_CALL_BYTES', call_bytes)
        del spy.calls[:]
        got = r.detect(1.0, sign='pos', exclude=0, spread=0)
        assert got.sample.size == ti.size
        assert got.sample.tobytes() == ti.astype(np.int64).tobytes() and got.channel.tobytes() == ji.astype(np.int64).tobytes()
        assert got.amplitude.tobytes() == np.full(ti.size, 7, np.float32).tobytes()
        caps = spy.caps()
        assert len(caps) == 2 * n_parts, caps                                   # every part: a short buffer, then room for all
        assert all(a < b for a, b in zip(caps[::2], caps[1::2])) and sum(caps[1::2]) == ti.size


# ---- 4. slab seams on plateaus and ties ------------------------------------------------------------------------------------------------
SEAM_BASE, SEAM_THR = 20, 50.0


def seam_recording(R):
    """int16, 5 columns, every sample SEAM_BASE except: in columns 0 / 1 (the first half of the distances) and 2 / 3 (the second), for
    every d in 1 .. R + 1 two equal peaks d rows apart, more than R rows from any other peak of their column; then, in column 4, a
    plateau of 2 R + 3 rows, a peak with a larger one R rows after it, and one with a larger one R + 1 rows after it.  At most two
    columns hold a peak in any row, so the median of every row is SEAM_BASE and the ties are ties with the reference too -- and a
    reference subtracted twice from a halo row breaks them.  -> (x, {name: rows} for the literal expectations, first row of the tail)."""
    G = R + 2
    cur = [0, 0, 0, 0]
    ds = list(range(1, R + 2))
    place = {}
    half = (len(ds) + 1) // 2
    for k, d in enumerate(ds):                                        # columns 0, 1 run side by side; 2, 3 follow after them
        c = (k % 2) + (2 if k >= half else 0)
        place[d] = (c, cur[c] + G)
        cur[c] = cur[c] + G + d
    shift = max(cur[0], cur[1])
    for d, (c, p) in list(place.items()):
        if c >= 2:
            place[d] = (c, p + shift)
    tail = shift + max(cur[2], cur[3]) + G
    plateau = tail
    small_r = plateau + 2 * R + 3 + G
    small_r1 = small_r + R + G
    rows = small_r1 + R + 1 + G + 3
    x = np.full((rows, 5), SEAM_BASE, np.int16)
    for d, (c, p) in place.items():
        x[p, c] = x[p + d, c] = SEAM_BASE + 1000 + d
    x[plateau:plateau + 2 * R + 3, 4] = SEAM_BASE + 800
    x[small_r, 4], x[small_r + R, 4] = SEAM_BASE + 500, SEAM_BASE + 900
    x[small_r1, 4], x[small_r1 + R + 1, 4] = SEAM_BASE + 500, SEAM_BASE + 900
    assert ((x != SEAM_BASE).sum(axis=1) <= 2).all()
    marks = dict(pair_R=place[R], pair_R1=place[R + 1], plateau=plateau, small_r=small_r, small_r1=small_r1)
    return x, marks, tail


def seam_literals(got, R, marks):
    ev = pairs_of(got)
    c, p = marks['pair_R']
    assert (p, c) in ev and (p + R, c) not in ev                     # equal peaks R apart: the earlier survives
    c, p = marks['pair_R1']
    assert (p, c) in ev and (p + R + 1, c) in ev                     # R + 1 apart: both do
    p = marks['plateau']
    assert [t for t, j in sorted(ev) if j == 4 and p <= t < p + 2 * R + 3] == [p]
    p = marks['small_r']
    assert (p, 4) not in ev and (p + R, 4) in ev
    p = marks['small_r1']
    assert (p, 4) in ev and (p + R + 1, 4) in ev


def run_seams(make, R, monkeypatch, one_row_slabs_over=3000, brute=False):
    """Unsplit, then slabs that own 1, R - 1, R, R + 1 and 2 R + 1 rows, from two starts: one puts a seam on a chunk boundary, the
    other next to it.  own = 1 makes every row a seam: over the whole recording when it is short, else over the last
    `one_row_slabs_over` rows (the distances near R and the tail).  -> the number of slabbed calls made."""
    x, marks, tail = seam_recording(R)
    rows = x.shape[0]
    chunk = min(1001, max(16, (rows // 4) | 1))
    r, dec = make(x, chunk)
    cols = np.arange(5)
    n_calls = 0
    for reference in (None, 'median'):
        kw = dict(sign='pos', reference=reference, exclude=R, spread=0)
        plain_env(monkeypatch)
        whole, _ = check(r, dec, cols, SEAM_THR, brute=brute, **kw)
        seam_literals(whole, R, marks)
        assert whole.sample.size >= R + 4
        for own in sorted({1, max(1, R - 1), R, R + 1, 2 * R + 1}):
            lo = 0 if own > 1 or rows <= one_row_slabs_over else rows - one_row_slabs_over
            boundary = chunk * (1 + lo // chunk)                       # a chunk boundary inside the range
            assert lo < boundary < rows
            for off in (0, 1):                                        # a seam on the chunk boundary; a seam one row after it
                start = lo + (boundary - lo) % own + off
                assert (boundary + off - start) % own == 0 and rows - start > own          # more than one slab
                monkeypatch.setenv('MTS_DETECT_SLAB_BYTES', str(slab_bytes(5, own, R)))
                got, _ = check(r, dec, cols, SEAM_THR, start, None, **kw)
                keep = whole.sample >= start
                for key in ('sample', 'channel', 'amplitude'):
                    assert got[key].tobytes() == whole[key][keep].tobytes(), (R, reference, own, off, key)
                if start <= min(marks['pair_R'][1], marks['pair_R1'][1]):
                    seam_literals(got, R, marks)
                n_calls += 1
    plain_env(monkeypatch)
    r.close()
    return n_calls


# ---- 5. word seams and the spread --------------------------------------------------------------------------------------------------------
WORD_NS, WORD_SS, WORD_RS = (64, 65, 96, 128, 129), (1, 31, 32), (0, 2)
WORD_H, WORD_THR, WORD_STEP = 100, 50.0, 8                      # (blocks WORD_STEP rows apart: no block sees another within R <= 2)


def word_recording(nc=129):
    """int16, small noise; for every S and every j of {0, S, 63, 64, 127, 128, n - 1 - S, n - 1 for every n} a block of rows with the
    value WORD_H at (t, j), (t, j +- S), (t, j +- (S + 1)), (t - 1, j + S) and (t + 1, j - S), what falls outside left out; then two blocks
    for the literal expectations: (t, 63) and (t, 64) alone, and (t, 64) with (t + 1, 63).  -> (x, {name: t})."""
    blocks = []
    for S in WORD_SS:
        js = {0, S, 63, 64, 127, 128}
        for n in WORD_NS:
            js |= {n - 1 - S, n - 1}
        for j in sorted(v for v in js if 0 <= v < nc):
            blocks.append([(0, j), (0, j - S), (0, j + S), (0, j - S - 1), (0, j + S + 1), (-1, j + S), (1, j - S)])
    blocks.append([(0, 63), (0, 64)])
    blocks.append([(0, 64), (1, 63)])
    rows = WORD_STEP * (len(blocks) + 1)
    rs = np.random.RandomState(5)
    x = rs.randint(-3, 4, size=(rows, nc)).astype(np.int16)
    for k, cells in enumerate(blocks):
        t = WORD_STEP * (k + 1)
        for dt, j in cells:
            if 0 <= j < nc:
                x[t + dt, j] = WORD_H
    return x, dict(same_row=WORD_STEP * (len(blocks) - 1), next_row=WORD_STEP * len(blocks))


def run_words(r, dec, marks, ns=WORD_NS, brute=False):
    n_ev = 0
    for n in ns:
        cols = np.arange(n)
        for S in WORD_SS:
            for R in WORD_RS:
                got, _ = check(r, dec, cols, WORD_THR, brute=brute, sign='pos', exclude=R, spread=S)
                n_ev += got.sample.size
                if n >= 65:
                    ev = pairs_of(got)
                    t = marks['same_row']
                    assert (t, 63) in ev and (t, 64) not in ev                   # one row: the lower position wins
                    t = marks['next_row']
                    assert (t, 64) in ev and ((t + 1, 63) in ev) == (R == 0)     # two rows: the earlier row wins when it is in reach
    assert n_ev >= 100
    return n_ev


# ---- 6. v > threshold is strict, column by column ------------------------------------------------------------------------------------------
def threshold_recording():
    """float32, 3 columns, zeros except rows 4, 8, 12: the float32 below 0.1, float32(0.1) and the float32 above it, in every column;
    rows 20, 24, 28 the same negated."""
    a = np.float32(0.1)
    vals = [np.nextafter(a, np.float32(-1)), a, np.nextafter(a, np.float32(1))]
    x = np.zeros((32, 3), np.float32)
    for k, v in enumerate(vals):
        x[4 + 4 * k] = v
        x[20 + 4 * k] = -v
    return x, vals


def run_threshold(r, dec, vals, brute=False):
    below, a, above = vals
    assert below < a < above and float(a) != 0.1 and np.float32(0.1) == a
    cols = np.arange(3)
    per_column = np.array([a, above, below], np.float32)              # column 1 takes nothing; column 2 takes float32(0.1) too
    for thr, per_col in ((0.1, [[12], [12], [12]]), (per_column, [[12], [], [8, 12]])):
        for sign, shift in (('pos', [0]), ('neg', [16]), ('both', [0, 16])):
            got, _ = check(r, dec, cols, thr, brute=brute, sign=sign, exclude=0, spread=0)
            want = sorted((t + s, j) for j in range(3) for t in per_col[j] for s in shift)
            assert sorted(pairs_of(got)) == want, (sign, sorted(pairs_of(got)), want)
            assert got.sample.size == len(want)
