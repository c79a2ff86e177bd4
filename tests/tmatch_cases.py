"""The cases of tests/test_gpu_tmatch_edges.py (k_correlate, k_tmatch_best, k_tmatch_mask, k_tmatch_emit and the slabs of correlate_run /
tmatch_run on the MI355X) and of their CPU twins in tests/test_tmatch_cases.py (the numpy stand-ins TmatchOracleCodec /
CorrelateOracleCodec, the brute-force restatements at small shapes, and the properties of the inputs that make the cases reach what
they say): the inputs and the checks are the same code, only the codec behind the Reader and the sizes differ.  Every comparison is
of bytes -- (sample, template, score) of the events against tests/tmatch_oracle.events_of_scores, float32 scores against
tests/correlate_oracle.correlate or a literal expectation -- over the oracle codec's decode; no tolerance anywhere.

make(x, chunk_rows) -> (Reader, the oracle's decode) is the caller's: the GPU file opens one lane on device 0, the twins the stand-in."""
import numpy as np

from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.correlate_oracle import FILL, correlate, correlate_brute
from tests.cov_quantile_cases import recording  # noqa: F401  (the callers' make() is built on it)
from tests.detect_cases import FMAX, SUBNORMAL, TINY, scan_shape, spiky_int8
from tests.tmatch_oracle import events_of_scores, events_of_scores_brute

TAPS9 = np.random.RandomState(1).randn(9)
BELOW_ALL = -3e38                                              # a threshold under every finite score of these cases but -FLT_MAX


def ev_bytes(ev):
    return tuple(np.ascontiguousarray(a).tobytes() for a in ev)


def scores_of(dec, k, before=0, cols=None, taps=None, reference=None, i0=0, i1=None):
    """The oracle's scores of file rows [i0, i1) (default: the whole file), the columns `cols` chosen."""
    n = dec.shape[0]
    x = dec if cols is None else dec[:, np.asarray(cols)]
    return correlate(x, 0, 0, n, i0, n if i1 is None else i1, [1.0] if taps is None else taps, 1 if reference else 0, before, k)


def check_events(r, score, k, thr, R, i0=0, i1=None, before=0, brute=False):
    """Reader.match_templates (no filter, no reference, every column) on rows [i0, i1) against the definition over the whole file's
    scores, byte for byte.  -> (the Bunch, the oracle's arrays)."""
    i1 = score.shape[0] if i1 is None else i1
    want = events_of_scores(score, 0, i0, i1, thr, R)
    if brute:
        assert ev_bytes(want) == ev_bytes(events_of_scores_brute(score, 0, i0, i1, thr, R)), 'the two restatements differ'
    got = r.match_templates(k, thr, i0, i1, before=before, exclude=R)
    assert (got.sample.dtype, got.template.dtype, got.score.dtype) == (np.int64, np.int64, np.float32)
    assert got.sample.tobytes() == want[0].tobytes(), ('sample', got.sample.size, want[0].size, got.sample[:6], want[0][:6])
    assert got.template.tobytes() == want[1].tobytes(), ('template', got.template[:6], want[1][:6])
    assert got.score.tobytes() == want[2].tobytes(), ('score', got.score[:6], want[2][:6])
    return got, want


def check_scores(r, want, k, i0, i1, before, channels=slice(None), taps=None, reference=None):
    """Reader.correlate on rows [i0, i1) against the rows of `want` (the expectation over the whole file), byte for byte."""
    got = r.correlate(k, i0, i1, channels=channels, before=before, taps=taps, reference=reference)
    assert got.dtype == np.float32 and got.shape == want[i0:i1].shape
    bad = np.argwhere(got.view(np.uint32) != want[i0:i1].view(np.uint32))
    assert not len(bad), (len(bad), bad[:4].tolist(), [(got[t, o], want[i0 + t, o]) for t, o in bad[:4]])
    return got


def pairs_of(got):
    return set(zip(got.sample.tolist(), got.template.tolist()))


class Spy:
    """Around codec.match_templates: records every call's arguments and result, so that a test sees the buffer sizes the Reader chose,
    and can make the device call again with another max_events."""

    def __init__(self, monkeypatch, r):
        self.calls, self.orig = [], r.codec.match_templates
        monkeypatch.setattr(r.codec, 'match_templates', self)

    def __call__(self, *args, **kw):
        out = self.orig(*args, **kw)
        self.calls.append((args, kw, out))
        return out

    def caps(self):
        return [int(args[-1]) for args, _, _ in self.calls]

    def ranges(self):
        return [(int(args[12]), int(args[13])) for args, _, _ in self.calls]

    def with_cap(self, i, cap):
        """Call i once more with max_events = cap.  -> (status, n_events, row, template, score)."""
        args, kw, _ = self.calls[i]
        return self.orig(*(args[:-1] + (int(cap),)), **kw)


def plain_env(monkeypatch):
    """The library reads these with getenv on every call: unset, one piece and one slab hold a small recording."""
    for name in ('MTS_PIPE_BYTES', 'MTS_TMATCH_SLAB_BYTES', 'MTS_CORRELATE_SLAB_BYTES'):
        monkeypatch.delenv(name, raising=False)


def slab_bytes(n_cols, n_out, own, R, T):
    """MTS_TMATCH_SLAB_BYTES for which a slab owns `own` rows (TmatchSlabs of csrc/reduce_plan.h, inverted): the z slab holds them, R
    rows either side and their T - 1 neighbours, the score slab them and R either side, float32 both."""
    return 4 * max(n_cols * (own + 2 * R + T - 1), n_out * (own + 2 * R))


# ---- the identity trick -----------------------------------------------------------------------------------------------------------------
def identity(n):
    """(n, 1, n): template k is 1 at column k.  With no filter, no reference and before = 0, score[t, k] is the chain of fmaf(x[t, j],
    K[k, 0, j], acc) from +0 over j: +-0 products everywhere but j == k."""
    return np.eye(n, dtype=np.float32)[:, None, :].copy()


def scores_of_identity(x):
    """What correlate(identity) must give on the float32 recording x, by rule instead of by the chain: the bits of x where x is finite
    (a -0 comes out +0: -0 + +0); a row with exactly one infinity keeps it in its own column and is NaN (0x7fc00000) in every other
    (inf * 0); a row with two infinities, or with a NaN, is all NaN."""
    x = np.asarray(x, np.float32)
    s = x.copy()
    s[s == 0] = 0.0
    n_inf, nan = np.isinf(x).sum(axis=1), np.isnan(x).any(axis=1)
    one = (n_inf == 1) & ~nan
    s[one[:, None] & ~np.isinf(x)] = FILL
    s[(n_inf >= 2) | nan] = FILL
    return s


# ---- A. the compaction: k_tmatch_emit and the count / scan it shares with detect ----------------------------------------------------------
# A block of the bitmap is 1024 words = 65 536 rows (one bit per row); thread i of k_tmatch_emit takes words 4 i .. 4 i + 3 = 256 rows,
# wave w the rows 16 384 w .. 16 384 w + 16 383 of the block.
BLOCK_ROWS, WAVE_ROWS, THREAD_ROWS = 65536, 16384, 256
EMIT_K1 = np.ones((1, 1, 1), np.float32)
EMIT_K3 = np.array([1.0, -1.0, 0.5], np.float32).reshape(3, 1, 1)        # the scores x, -x, x / 2: template 0 where x > 0, 1 where x < 0
# (rows, chunk rows, rows a slab owns or None: one slab)
EMIT_CASES = [(16384, 40000, None), (16385, 40000, None),       # the last thread of wave 0; the first of wave 1
              (65536, 40000, None), (65537, 40000, None),       # one full block; a second block of one word
              (262145, 40000, None),                            # five blocks, the last of one word
              (2 * 262144 + 7, 50000, None),                    # nine blocks, the last thread that has rows ragged (7 rows)
              (2 * 262144 + 7, 50000, 262150)]                  # two slabs of five blocks: the second emit starts from the first's total
EMIT_CAPS = (lambda total: total - 1, lambda total: 65536, lambda total: 65537, lambda total: 16385, lambda total: 257, lambda total: 1,
             lambda total: 0)
# (threshold, exclude): sparse (the spikes, thinned); half dense (x > 0.5 for one template: the popcounts of the threads differ; |x| > 0.5
# for three: all rows but the zeros, the template varying); every row (every bit of every word)
EMIT_SPARSE, EMIT_HALF, EMIT_ALL = (105.0, 3), (0.5, 0), (BELOW_ALL, 0)


def emit_shape(rows):
    """(bitmap words, blocks of k_tmatch_emit, blocks per thread of k_detect_scan) of a slab that owns `rows` rows."""
    return scan_shape(-(-rows // 64), 1)


def emit_recording(rows, n_spikes=4000):
    """The last row is positive: where it is alone in its word, thread, wave or block, that one has an event to place."""
    x = spiky_int8(rows, 1, n_spikes, rows % 1000 + 1)
    x[-1, 0] = max(int(x[-1, 0]), 7)
    return x


def emit_events(x, k, check):
    """The oracle's events of one of the three checks on the whole recording x (the input's own property: nothing of the device)."""
    thr, R = check
    return events_of_scores(scores_of(x, k), 0, 0, x.shape[0], thr, R)


def run_emit(make, rows, chunk, own, monkeypatch, caps=EMIT_CAPS, dev=None, n_spikes=4000, brute=False):
    """Both template sets: the three checks over the whole range in one call each, the Reader's own two calls (a first buffer too
    small, the second exact); the half-dense device call again with the capacities `caps` (callables of the total); own: in slabs that
    own that many rows; dev(k, thr, R, cap) -> (n_events, (row, template, score)): the entry point that leaves the results on the
    device.  -> {templates: (sparse, half-dense, every-row events)}."""
    x = emit_recording(rows, n_spikes)
    r, dec = make(x, chunk)
    monkeypatch.setattr(api, 'TMATCH_GUESS_MIN', 16)
    spy = Spy(monkeypatch, r)
    out = {}
    for k in (EMIT_K1, EMIT_K3):
        score = scores_of(dec, k)
        sizes = []
        for thr, R in (EMIT_SPARSE, EMIT_HALF, EMIT_ALL):
            plain_env(monkeypatch)
            if own:
                monkeypatch.setenv('MTS_TMATCH_SLAB_BYTES', str(slab_bytes(1, len(k), own, R, 1)))
            del spy.calls[:]
            _, want = check_events(r, score, k, thr, R, brute=brute)
            total = want[0].size
            sizes.append(total)
            if (thr, R) == EMIT_SPARSE:
                continue
            # the Reader's own two calls: one part over the whole range, a first buffer too small, the second exact
            assert spy.ranges() == [(0, rows)] * 2, spy.ranges()
            assert spy.caps() == [max(api.TMATCH_GUESS_MIN, rows // api.TMATCH_GUESS_SAMPLES), total] and spy.caps()[0] < total
            full = spy.calls[1][2]
            assert full[1] == total and full[2].size == total
            if (thr, R) != EMIT_HALF:
                assert total == rows and want[0].tobytes() == np.arange(rows, dtype=np.int64).tobytes()
                continue
            for cap in [c(total) for c in caps]:
                st, n_ev, row, tpl, val = spy.with_cap(0, cap)
                assert all(s == hip.CHUNK_OK for s in st) and n_ev == total and row.size == tpl.size == val.size == min(cap, total), cap
                assert ev_bytes((row, tpl, val)) == ev_bytes(v[:cap] for v in full[2:]), cap
            if dev is not None:
                for cap in (total, 65537):
                    n_ev, res = dev(k, thr, R, cap)
                    assert n_ev == total and ev_bytes((res[0], res[1].astype(np.int64), res[2])) == ev_bytes(v[:cap] for v in want), cap
        out[len(k)] = tuple(sizes)
    plain_env(monkeypatch)
    r.close()
    return out


# ---- B. the row maxima: k_tmatch_best by the identity trick ---------------------------------------------------------------------------------
BEST_NS = (64, 65, 1023, 1024)
# index rows: the maximum of row i sits at column i; its class is i % 3 -- an event (the threshold of template i is the float32 below the
# value), none (the value itself), none (the float32 above it).  The values of the classes differ so that a threshold read from another
# class turns the verdict: a row of class 0 read against a threshold of class 1 or 2 is no event, a row of class 1 or 2 read against one of
# class 0 is one -- thr[0] read for every template makes every row an event, thr[i - 1] or thr[i + 1] turns two rows of three.  (No single
# vector lets EVERY other entry turn EVERY row: of two event rows, each one's threshold would have to be at or above the other's value
# and below its own.)
POS_VALUES, NEG_VALUES = (1.0, 3.0, 3.0), (-0.75, -0.25, -0.25)       # by class; the base of a row is random in [-2, -1)
TIE, NEG_TIE = 2.0, -0.5


def _near(v):
    v = np.float32(v)
    return np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))


def best_thresholds(n, values):
    """thr[i] for the index rows whose maxima are values[i % 3]."""
    return np.array([_near(values[i % 3])[i % 3] for i in range(n)], np.float32)


def tie_pairs(n):
    """(first index, second index) of two equal maxima: one lane (i, i + 64); neighbours; the wave's seam; both ends; and the lower
    index on the higher lane (64 a + 6, 64 b + 5 with a < b: lanes 6 and 5), where n has room."""
    pairs = [(i, i + 64) for i in (0, 5, 63, 64, n - 129, n - 65)] + [(i, i + 1) for i in (0, 5, 62, 63, 64, 127, n - 2)]
    pairs += [(63, 64), (0, n - 1), (70, 133), (6, 64 * ((n - 6) // 64) + 5), (6 + 64 * ((n - 70) // 128), 64 * ((n - 6) // 64) + 5), (6, 69)]
    return sorted({(a, b) for a, b in pairs if 0 <= a < b < n})


def best_recording(n):
    """float32, n columns: the score matrix that the identity templates read back.  -> (x, marks): marks[name] = (first row, stop row)
    of a family, marks['ties'] = [(row, first index)], marks['inf'] = [(row, column)], marks['none'] = rows without an event under any
    threshold, marks['events'] = [(row, template)] of the other special rows under the threshold BELOW_ALL, marks['sub'] = [(row,
    template or None)] under the threshold 0."""
    rs = np.random.RandomState(n)
    rows, marks = [], dict(ties=[], inf=[], none=[], events=[], sub=[])

    def base():
        return rs.uniform(-2.0, -1.0, n).astype(np.float32)

    def put(row):
        rows.append(np.asarray(row, np.float32))
        return len(rows) - 1

    def col(j):
        return j % n
    for name, values in (('pos', POS_VALUES), ('neg', NEG_VALUES)):
        first = len(rows)
        for i in range(n):
            row = base()
            row[i] = values[i % 3]
            put(row)
        marks[name] = (first, len(rows))
    for a, b in tie_pairs(n):
        for v in (TIE, NEG_TIE):
            row = base()
            row[[a, b]] = v
            marks['ties'].append((put(row), a))
    marks['ties'].append((put(np.full(n, TIE)), 0))                    # a constant row
    marks['ties'].append((put(np.full(n, NEG_TIE)), 0))
    for j in sorted({0, 63 % n, 64 % n, n - 1}):                       # one +inf: every other score of the row is NaN
        row = base()
        row[j] = np.inf
        marks['inf'].append((put(row), j))
    row = base()
    row[col(5)] = -np.inf                                              # one -inf: the row's maximum, and no event
    marks['none'].append(put(row))
    row = base()
    row[[col(1), col(2)]] = [np.inf, -np.inf]                          # two infinities: all NaN
    marks['none'].append(put(row))
    row = base()
    row[col(1)] = row[col(3)] = np.inf
    marks['none'].append(put(row))
    row = base()
    row[col(3)] = np.nan                                               # one NaN: all NaN
    marks['none'].append(put(row))
    row = base()
    row[col(7)] = FMAX
    marks['events'].append((put(row), col(7)))
    marks['none'].append(put(np.full(n, -FMAX)))                       # (no finite threshold lies below it)
    row = np.full(n, -FMAX)
    row[col(11)] = -1.5
    marks['events'].append((put(row), col(11)))
    row = base()
    row[col(13)] = SUBNORMAL                                           # subnormal maxima: above the threshold 0, and below it
    marks['events'].append((put(row), col(13)))
    marks['sub'].append((len(rows) - 1, col(13)))
    row = base()
    row[col(14)] = -SUBNORMAL
    marks['events'].append((put(row), col(14)))
    marks['sub'].append((len(rows) - 1, None))
    row = np.zeros(n)
    row[::2] = -0.0
    row[col(15)] = 1000 * SUBNORMAL
    marks['events'].append((put(row), col(15)))
    marks['sub'].append((len(rows) - 1, col(15)))
    a, b = tie_pairs(n)[-1]
    row = np.full(n, -TINY)
    row[[a, b]] = 3 * SUBNORMAL                                        # a tie of subnormals over the largest negative normal
    marks['events'].append((put(row), a))
    marks['sub'].append((len(rows) - 1, a))
    row = base()
    row[[col(4), col(5)]] = [-0.0, 0.0]                                # -0 == +0: the first of them, and its score is +0
    marks['events'].append((put(row), col(4)))
    marks['sub'].append((len(rows) - 1, None))
    return np.array(rows, np.float32), marks


def best_literals(marks, n, family, got):
    """The events of the index rows `family` under best_thresholds: the rows of class 0, each with its own index and value."""
    first, stop = marks[family]
    values = POS_VALUES if family == 'pos' else NEG_VALUES
    idx = np.arange(0, n, 3)
    assert stop - first == n
    assert got.sample.tolist() == (first + idx).tolist() and got.template.tolist() == idx.tolist()
    assert got.score.tobytes() == np.full(idx.size, values[0], np.float32).tobytes()


def special_literals(marks, n, got, thr):
    """The events of every row under one threshold for all templates: BELOW_ALL or 0."""
    ev = pairs_of(got)
    rows = set(got.sample.tolist())
    for name in ('pos', 'neg'):
        first, stop = marks[name]
        want = [(first + i, i) for i in range(n)] if thr < -1 or name == 'pos' else []
        assert sorted(e for e in ev if first <= e[0] < stop) == want, name
    for i, (t, a) in enumerate(marks['ties']):                        # (positive and negative ties take turns)
        assert ((t, a) in ev) if thr < -1 or i % 2 == 0 else (t not in rows), (t, a)
    assert all((t, j) in ev for t, j in marks['inf'])
    assert not rows & set(marks['none'])
    if thr < -1:
        assert all(e in ev for e in marks['events'])
    else:
        assert all(((t, a) in ev) if a is not None else (t not in rows) for t, a in marks['sub'])


def run_best(make, n, brute=False):
    """The recording in chunks of 64 rows: correlate(identity) reads it back bit for bit; the index rows against their per-template
    thresholds, both families; every row against BELOW_ALL and against 0.  exclude = 0: every row stands alone.
    -> the templates seen in an event."""
    x, marks = best_recording(n)
    r, dec = make(x, 64)
    k = identity(n)
    score = scores_of_identity(dec)
    check_scores(r, score, k, 0, len(x), 0)
    seen = set()
    for family, values in (('pos', POS_VALUES), ('neg', NEG_VALUES)):
        first, stop = marks[family]
        got, _ = check_events(r, score, k, best_thresholds(n, values), 0, first, stop, brute=brute)
        best_literals(marks, n, family, got)
    for thr in (BELOW_ALL, 0.0):
        got, _ = check_events(r, score, k, thr, 0, brute=brute)
        special_literals(marks, n, got, thr)
        seen |= set(got.template.tolist())
    r.close()
    return seen


# ---- C. slab seams of the mask on plateaus and ties -------------------------------------------------------------------------------------------
SEAM_N, SEAM_BASE, SEAM_THR = 4, 1.0, 50.0


def seam_recording(R):
    """float32, 4 columns read back by the identity templates, every score SEAM_BASE except: for every d in 1 .. R + 1 two equal peaks d
    rows apart, more than R rows from any other peak -- once both on template 2, once the later row on the lower template (2, then 1);
    then two equal peaks in one row (templates 1 and 3), a plateau of 2 R + 3 rows on template 3, a peak with a larger one R rows after
    it, and one with a larger one R + 1 rows after it (template 0).  -> (x, {name: row} for the literal expectations)."""
    G = R + 2
    same_row = G                                                   # the tail first: the last rows are the distances near R
    plateau = same_row + G
    small_r = plateau + 2 * R + 3 + G
    small_r1 = small_r + R + G
    at, t, pairs = {}, small_r1 + R + 1 + G, []
    for d in range(1, R + 2):
        for kind, (ka, kb) in (('same', (2, 2)), ('cross', (2, 1))):
            at[(kind, d)] = t
            pairs.append((t, ka, t + d, kb, 1000.0 + d))
            t += d + G
    rows = t + 3
    x = np.full((rows, SEAM_N), SEAM_BASE, np.float32)
    for ta, ka, tb, kb, v in pairs:
        x[ta, ka] = x[tb, kb] = v
    x[same_row, [1, 3]] = 700.0
    x[plateau:plateau + 2 * R + 3, 3] = 800.0
    x[small_r, 0], x[small_r + R, 0] = 500.0, 900.0
    x[small_r1, 0], x[small_r1 + R + 1, 0] = 500.0, 900.0
    marks = dict(same_R=at[('same', R)], cross_R=at[('cross', R)], same_R1=at[('same', R + 1)], cross_R1=at[('cross', R + 1)],
                 same_row=same_row, plateau=plateau, small_r=small_r, small_r1=small_r1)
    return x, marks


def seam_literals(got, R, marks):
    ev = pairs_of(got)
    p = marks['same_R']
    assert (p, 2) in ev and (p + R, 2) not in ev                      # equal peaks R apart: the earlier survives ...
    p = marks['cross_R']
    assert (p, 2) in ev and (p + R, 1) not in ev                      # ... also against a lower template
    p = marks['same_R1']
    assert (p, 2) in ev and (p + R + 1, 2) in ev                      # R + 1 apart: both do
    p = marks['cross_R1']
    assert (p, 2) in ev and (p + R + 1, 1) in ev
    p = marks['same_row']
    assert (p, 1) in ev and (p, 3) not in ev                          # one row: the lower template
    p = marks['plateau']
    assert [e for e in sorted(ev) if p <= e[0] < p + 2 * R + 3] == [(p, 3)]
    p = marks['small_r']
    assert (p, 0) not in ev and (p + R, 0) in ev
    p = marks['small_r1']
    assert (p, 0) in ev and (p + R + 1, 0) in ev


def seam_events(x, R, brute=False):
    """The oracle's events of the seam recording (by the rule of the identity trick), as a Bunch."""
    fn = events_of_scores_brute if brute else events_of_scores
    row, tpl, val = fn(scores_of_identity(x), 0, 0, len(x), SEAM_THR, R)
    return api.Bunch(sample=row, template=tpl, score=val)


def run_seams(make, R, monkeypatch, one_row_slabs_over=3000, brute=False):
    """Unsplit, then slabs that own 1, R - 1, R, R + 1 and 2 R + 1 rows, from two starts: one puts a seam on a chunk boundary, the other
    next to it.  own = 1 makes every row a seam: over the whole recording when it is short, else over the last `one_row_slabs_over`
    rows (the distances near R).  -> the number of slabbed calls made."""
    x, marks = seam_recording(R)
    rows = x.shape[0]
    chunk = min(1001, max(16, (rows // 4) | 1))
    r, dec = make(x, chunk)
    k = identity(SEAM_N)
    score = scores_of_identity(dec)
    n_calls = 0
    plain_env(monkeypatch)
    whole, _ = check_events(r, score, k, SEAM_THR, R, brute=brute)
    seam_literals(whole, R, marks)
    assert whole.sample.size == 2 * R + 9                             # a pair: one event up to R apart, two at R + 1; five in the tail
    for own in sorted({1, max(1, R - 1), R, R + 1, 2 * R + 1}):
        lo = 0 if own > 1 or rows <= one_row_slabs_over else rows - one_row_slabs_over
        boundary = chunk * (1 + lo // chunk)                           # a chunk boundary inside the range
        assert lo < boundary < rows
        for off in (0, 1):                                            # a seam on the chunk boundary; a seam one row after it
            start = lo + (boundary - lo) % own + off
            assert (boundary + off - start) % own == 0 and rows - start > own          # more than one slab
            monkeypatch.setenv('MTS_TMATCH_SLAB_BYTES', str(slab_bytes(SEAM_N, SEAM_N, own, R, 1)))
            got, _ = check_events(r, score, k, SEAM_THR, R, start, None)
            keep = whole.sample >= start
            for key in ('sample', 'template', 'score'):
                assert got[key].tobytes() == whole[key][keep].tobytes(), (R, own, off, key)
            if start <= min(marks.values()):
                seam_literals(got, R, marks)
            n_calls += 1
    plain_env(monkeypatch)
    r.close()
    return n_calls


# ---- D. template streaming and the limits of k_correlate ----------------------------------------------------------------------------------
# a chunk of the templates is 16 taus: T either side of one, two and three chunks, an exact multiple, and the last ragged row
EDGE_TS = (15, 16, 17, 31, 32, 33, 48, 255)
EDGE_SHAPES = ((4, 3), (5, 70), (20, 70))                      # (n_cols, n_out): one group; two groups, two output tiles; two bands, two tiles
EDGE_ROWS, EDGE_CHUNK = 130, 65


def edge_shapes(T):
    return ((5, 70),) if T == 255 else EDGE_SHAPES             # (the numpy chain of 255 taus stays short)


def edge_recording():
    return synth_int16(0, EDGE_ROWS, 70, 6)


def edge_case(dec, T, n_cols, n_out, before, i0=0, i1=None, brute=False):
    """-> (templates, columns, the oracle's scores of file rows [i0, i1): TAPS9 and the median reference)."""
    rs = np.random.RandomState(1000 * T + 10 * n_cols + n_out)
    k = rs.randn(n_out, T, n_cols).astype(np.float32)
    cols = [int(c) for c in rs.permutation(70)[:n_cols]]
    want = scores_of(dec, k, before, cols, TAPS9, 'median', i0, i1)
    if brute:
        n = dec.shape[0]
        other = correlate_brute(dec[:, cols], 0, 0, n, i0, n if i1 is None else i1, TAPS9, 1, before, k)
        assert other.tobytes() == want.tobytes(), 'the two restatements differ'
    return k, cols, want


def run_chunk_edges(r, dec, T):
    for n_cols, n_out in edge_shapes(T):
        for before in (0, T):
            k, cols, want = edge_case(dec, T, n_cols, n_out, before)
            for i0, i1 in ((0, EDGE_ROWS), (5, EDGE_ROWS - 1)):
                check_scores(r, want, k, i0, i1, before, cols, TAPS9, 'median')


LIMIT_SHAPES = ((1024, 1, 2), (1023, 2, 1), (4, 1024, 3), (7, 1023, 2))       # (n_cols, n_out, T): 64 bands; 16 output tiles, kp = 1024
LIMIT_ROWS = 70
TALL = (17, 65, 256)                                           # 64 + 255 staged rows with two bands and two output tiles
TALL_ROWS, TALL_CHUNK = 400, 100


def run_limit(r, dec, n_cols, n_out, T):
    """No reference (the median has its own column limit); the columns drawn with repeats from the recording's 70."""
    rs = np.random.RandomState(n_cols + n_out + T)
    k = rs.randn(n_out, T, n_cols).astype(np.float32)
    cols = [int(c) for c in rs.randint(0, dec.shape[1], n_cols)]
    want = scores_of(dec, k, T // 2, cols, TAPS9, None)
    check_scores(r, want, k, 0, dec.shape[0], T // 2, cols, TAPS9, None)
    check_scores(r, want, k, 3, dec.shape[0] - 1, T // 2, cols, TAPS9, None)


def run_tall(r, dec, before, part=(70, 333)):
    n_cols, n_out, T = TALL
    rs = np.random.RandomState(before)
    k = rs.randn(n_out, T, n_cols).astype(np.float32)
    cols = [int(c) for c in rs.permutation(dec.shape[1])[:n_cols]]
    want = scores_of(dec, k, before, cols, TAPS9, 'median')
    check_scores(r, want, k, 0, dec.shape[0], before, cols, TAPS9, 'median')
    check_scores(r, want, k, part[0], part[1], before, cols, TAPS9, 'median')


# the impulse read-out: every template entry comes back by name
IMP_COLS, IMP_OUT, IMP_T, IMP_STEP = 20, 65, 256, 260


def impulse_rows():
    return [IMP_T + IMP_STEP * j for j in range(IMP_COLS)]


def impulse_recording():
    x = np.zeros((impulse_rows()[-1] + 10, IMP_COLS), np.float32)
    for j, t in enumerate(impulse_rows()):
        x[t, j] = 2.0
    return x


def impulse_templates():
    k, tau, j = np.meshgrid(np.arange(IMP_OUT), np.arange(IMP_T), np.arange(IMP_COLS), indexing='ij')
    v = 1 + k + IMP_OUT * (tau + IMP_T * j)
    assert v.max() < 2 ** 24                                    # exact in float32, and so is twice it
    return v.astype(np.float32)


def impulse_scores(i0=0, i1=None):
    """score[t_j - tau, k] == 2 K[k, tau, j]; every other score is +0 (before = 0).  Rows [i0, i1)."""
    K = impulse_templates()
    rows = impulse_rows()[-1] + 10
    want = np.zeros((rows, IMP_OUT), np.float32)
    for j, t in enumerate(impulse_rows()):
        want[t - IMP_T + 1:t + 1] = 2 * K[:, ::-1, j].T
    return want[i0:rows if i1 is None else i1]


def impulse_first_mismatch(got, want, i0=0):
    """None, or the first score that differs as (row, (k, tau, j) of the template entry it should hold or None, got, wanted)."""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if not len(bad):
        return None
    t, k = int(bad[0][0]) + i0, int(bad[0][1])
    name = None
    for j, tj in enumerate(impulse_rows()):
        if tj - IMP_T < t <= tj:
            name = (k, tj - t, j)
    return t, name, float(got[t - i0, k]), float(want[t - i0, k])


def run_impulse(r):
    got = r.correlate(impulse_templates(), before=0)
    want = impulse_scores()
    assert got.shape == want.shape
    assert impulse_first_mismatch(got, want) is None, 'row, (k, tau, j), got, wanted: %r' % (impulse_first_mismatch(got, want),)


# subnormal operands: 200 rows x 9 columns, T = 5, 6 templates
SUB_ROWS, SUB_COLS, SUB_T, SUB_OUT, SUB_BEFORE = 200, 9, 5, 6, 2


def _magnitudes(rs, lo, hi, shape):
    return (10.0 ** rs.uniform(lo, hi, shape)) * rs.choice([-1.0, 1.0], shape)


def subnormal_case(kind):
    """-> (x float32, templates float32, columns).  'x': subnormal x against large templates; 'k': large x against templates that are
    subnormal in float32; 'both': both subnormal -- every product underflows to +-0.  In 'both' the first 8 columns are taken: with 9
    the chain ends on the +0 products of the padding columns 9 .. 11 and every score is +0; with 8 there is no padding, and a score
    has the sign of the last product."""
    rs = np.random.RandomState(('x', 'k', 'both').index(kind))
    small, large = (-42, -39), (20, 25)
    x = _magnitudes(rs, *(small if kind in ('x', 'both') else large), (SUB_ROWS, SUB_COLS)).astype(np.float32)
    k = _magnitudes(rs, *(small if kind in ('k', 'both') else large), (SUB_OUT, SUB_T, SUB_COLS)).astype(np.float32)
    cols = list(range(8 if kind == 'both' else SUB_COLS))
    return x, k[:, :, :len(cols)].copy(), cols


def is_subnormal(a):
    a = np.abs(a)
    return (a > 0) & (a < TINY)


def run_subnormal(make, kind):
    """-> the oracle's scores."""
    x, k, cols = subnormal_case(kind)
    r, dec = make(x, 100)
    want = scores_of(dec, k, SUB_BEFORE, cols)
    check_scores(r, want, k, 0, SUB_ROWS, SUB_BEFORE, cols)
    r.close()
    return want
