"""The cases of tests/test_gpu_tmatch_edges.py (tests/tmatch_cases.py) on the CPU: the same run_* helpers through the numpy stand-ins
(TmatchOracleCodec / CorrelateOracleCodec), with the brute-force restatements beside them where they are cheap, and the properties of
the inputs that make the cases reach what the GPU file says they reach -- computed from the oracle's scores and events, never from a
device.  Where the full size is slow in numpy a test says how it is reduced."""
import numpy as np
import pytest

from mtscomp_amd import api
from tests import tmatch_cases as K
from tests.correlate_oracle import CorrelateOracleCodec, correlate
from tests.tmatch_oracle import TmatchOracleCodec, events_of_scores


class BothOracleCodec(TmatchOracleCodec, CorrelateOracleCodec):
    """One stand-in with correlate and match_templates."""


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    K.plain_env(monkeypatch)
    return tmp_path


def _make(tmp):
    return lambda x, chunk_rows: K.recording(tmp, x, chunk_rows, codec=BothOracleCodec(n_lanes=1, capacity_chunks=8))


def _bunch(ev):
    return api.Bunch(sample=ev[0], template=ev[1], score=ev[2])


def test_slab_bytes_inverts_the_plan():
    """TmatchSlabs (csrc/reduce_plan.h) restated: own = min(bytes / (4 n_cols) - 2 R - (T - 1), bytes / (4 n_out) - 2 R)."""
    for n_cols, n_out, T in ((1, 1, 1), (1, 3, 1), (4, 4, 1), (20, 10, 61), (3, 70, 5)):
        for R in (0, 1, 7, 255):
            for own in (1, 2, R + 1, 2 * R + 1, 262150):
                b = K.slab_bytes(n_cols, n_out, own, R, T)
                assert min(b // (4 * n_cols) - 2 * R - (T - 1), b // (4 * n_out) - 2 * R) == own
                assert min((b - 1) // (4 * n_cols) - 2 * R - (T - 1), (b - 1) // (4 * n_out) - 2 * R) == own - 1


# ---- A ------------------------------------------------------------------------------------------------------------------------------------
EMIT_BLOCKS = {16384: 1, 16385: 1, 65536: 1, 65537: 2, 262145: 5, 262150: 5, 2 * 262144 + 7: 9}


@pytest.mark.parametrize('rows', sorted({c[0] for c in K.EMIT_CASES}))
def test_emit_cases_reach_what_they_say(rows):
    """The geometry: one bit per row, so a block of 1024 words is 65 536 rows and these recordings have 1 .. 9 blocks.  (A slab of
    match_templates owns at most 2^22 rows = 64 blocks: the second block per thread of k_detect_scan, past 256 blocks, is out of its
    reach, and stays with tests/test_gpu_detect_edges.py.)  The densities: of the oracle's events of the whole recording."""
    words, blocks, per = K.emit_shape(rows)
    assert (words, blocks, per) == (-(-rows // 64), EMIT_BLOCKS[rows], 1)
    owns = [c[2] for c in K.EMIT_CASES if c[0] == rows and c[2]]
    for own in owns:
        assert [K.emit_shape(own)[1], K.emit_shape(rows - own)[1]] == [EMIT_BLOCKS[own], EMIT_BLOCKS[rows - own]] == [5, 5]
    x = K.emit_recording(rows)
    for k in (K.EMIT_K1, K.EMIT_K3):
        sparse, half, every = (K.emit_events(x, k, c)[0] for c in (K.EMIT_SPARSE, K.EMIT_HALF, K.EMIT_ALL))
        assert every.size == rows
        # the spikes: 4000 draws, of either sign; one template sees the positive ones only, and at 16 384 rows one row in four is a
        # spike and many have a larger neighbour within 3 rows -- 2000 .. 4000 events where both signs count and the spikes are sparse
        print('rows %d, %d templates: sparse %d, half dense %d' % (rows, len(k), sparse.size, half.size))
        if len(k) == 3 and rows >= 65536:
            assert 2000 <= sparse.size <= 4000
        assert 900 <= sparse.size <= 4000
        assert (0.45 if len(k) == 1 else 0.99) * rows <= half.size < rows
        thread = np.bincount(half // K.THREAD_ROWS, minlength=-(-rows // K.THREAD_ROWS))
        if rows >= 16385:
            first = thread[:K.BLOCK_ROWS // K.THREAD_ROWS]
            waves = np.add.reduceat(first, np.arange(0, first.size, 64))
            assert (waves > 0).all() and waves.size == min(4, -(-rows // K.WAVE_ROWS))     # every wave of block 0 that has rows
            assert len(set(first[:-1].tolist())) > 1                                      # the popcounts of its threads differ
        if rows >= 65537:
            assert (np.bincount(half // K.BLOCK_ROWS) > 0).sum() == blocks >= 2
            assert (half >= K.BLOCK_ROWS + K.WAVE_ROWS).any() or rows < K.BLOCK_ROWS + K.WAVE_ROWS
        for own in owns:                # the second slab's emit starts from the first's total: past 2^17 with every row an event, and
            assert own > 2 ** 17        # half dense with three templates (with one it is just below: half of 262 150)
            assert ((half < own).sum() > 2 ** 17) == (len(k) == 3) and (half < own).sum() > 130000


def test_emit_case_and_capacities_on_the_stand_in(tmp_cfg, monkeypatch):
    """Reduced: 3000 rows with 300 spikes in chunks of 1000 (numpy's brute force beside it), the capacities that are below the total."""
    out = K.run_emit(_make(tmp_cfg), 3000, 1000, None, monkeypatch, caps=K.EMIT_CAPS[:1] + K.EMIT_CAPS[4:], n_spikes=300, brute=True)
    assert out[1][2] == out[3][2] == 3000 and 50 <= out[1][0] < out[3][0] <= 300 and out[1][1] < out[3][1]


# ---- B ------------------------------------------------------------------------------------------------------------------------------------
def _chain(x):
    n = x.shape[1]
    return correlate(x, 0, 0, len(x), 0, len(x), [1.0], 0, 0, K.identity(n))


@pytest.mark.parametrize('n', [8, 68, 1024])
def test_identity_rule_is_the_chain(n):
    """scores_of_identity against the fmaf chain, byte for byte: every row family at n = 8 and 68; at n = 1024, where the chain costs
    seconds per 70 rows, on 64 rows: the special ones and a sample of the index rows."""
    x, marks = K.best_recording(n)
    if n == 1024:
        special = np.arange(marks['neg'][1], len(x))
        some = np.random.RandomState(0).choice(marks['neg'][1], 64 - min(40, special.size), replace=False)
        x = x[np.r_[some, special[-40:]]]
        assert len(x) == 64
    assert np.isinf(x).any() and np.isnan(x).any() and (np.signbit(x) & (x == 0)).any()
    assert K.scores_of_identity(x).tobytes() == _chain(x).tobytes()
    if n == 8:
        for R in (1, 7):
            s = K.seam_recording(R)[0]
            assert K.scores_of_identity(s).tobytes() == s.tobytes() == correlate(s, 0, 0, len(s), 0, len(s), [1.0], 0, 0, K.identity(4)).tobytes()


@pytest.mark.parametrize('n', K.BEST_NS)
def test_best_recording_is_what_it_says(n):
    """By the oracle alone, at every width of the GPU test: every index is the template of some event, every tie row's event carries the
    first index, the three thresholds give event / none / none, and a threshold read from a neighbouring template turns the verdict."""
    x, marks = K.best_recording(n)
    score = K.scores_of_identity(x)
    for family, values in (('pos', K.POS_VALUES), ('neg', K.NEG_VALUES)):
        first, stop = marks[family]
        thr = K.best_thresholds(n, values)
        ev = events_of_scores(score, 0, first, stop, thr, 0)
        K.best_literals(marks, n, family, _bunch(ev))
        below, at, above = K._near(values[0])
        assert below < at < above and thr[0] == below and thr[1] == np.float32(values[1]) and thr[2] > np.float32(values[2])
        for shift, same in ((1, 2), (-1, 1)):                           # thr[i - 1] / thr[i + 1] read instead of thr[i]: the verdict turns
            wrong = set(events_of_scores(score, 0, first, stop, np.roll(thr, shift), 0)[0].tolist())      # but for one class of three
            mine = set(ev[0].tolist())
            edge = {first, stop - 1}                                    # (the roll wraps the ends around)
            assert all(((t in mine) != (t in wrong)) == ((t - first) % 3 != same) for t in range(first, stop) if t not in edge)
        wrong = events_of_scores(score, 0, first, stop, np.full(n, thr[0]), 0)[0]             # thr[0] for every template: every row
        assert wrong.size == n
    tie_rows = dict(marks['ties'])
    seen = set()
    for thr in (K.BELOW_ALL, 0.0):
        ev = events_of_scores(score, 0, 0, len(x), thr, 0)
        K.special_literals(marks, n, _bunch(ev), thr)
        seen |= set(ev[1].tolist())
        assert all(tie_rows[t] == a for t, a in zip(ev[0].tolist(), ev[1].tolist()) if t in tie_rows)
    assert seen == set(range(n))
    lanes = [(a, b) for a, b in K.tie_pairs(n) if a % 64 > b % 64]
    assert ((70, 133) in lanes and len(lanes) >= 4) if n >= 134 else lanes == [(63, 64)][:n - 64]       # the lower index on the higher lane
    assert any(b - a == 64 for a, b in K.tie_pairs(n)) == (n > 64)


@pytest.mark.parametrize('n', [8, 64, 65])
def test_row_maxima_on_the_stand_in(tmp_cfg, n):
    """Reduced: 8 (with numpy's brute force), 64 and 65 templates; the chain at 1023 and 1024 costs minutes."""
    assert K.run_best(_make(tmp_cfg), n, brute=n == 8) == set(range(n))


# ---- C ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', [1, 7])
def test_slab_seam_recording_on_the_stand_in(tmp_cfg, monkeypatch, R):
    assert K.run_seams(_make(tmp_cfg), R, monkeypatch, brute=True) >= 6


@pytest.mark.parametrize('R', [1, 7, 255])
def test_slab_seam_literals_hold(R):
    """Every literal of the seam list, in both restatements (the brute force on R <= 7 only: it is quadratic in R)."""
    x, marks = K.seam_recording(R)
    got = K.seam_events(x, R)
    K.seam_literals(got, R, marks)
    assert got.sample.size == 2 * R + 9
    if R <= 7:
        K.seam_literals(K.seam_events(x, R, brute=True), R, marks)
    else:
        assert len(x) - marks['same_R'] < 3000 < len(x)                 # the one-row slabs run over the distances R and R + 1


# ---- D ------------------------------------------------------------------------------------------------------------------------------------
def _edge_reader(tmp):
    return _make(tmp)(K.edge_recording(), K.EDGE_CHUNK)


@pytest.mark.parametrize('T', K.EDGE_TS)
def test_chunk_edges_on_the_stand_in(tmp_cfg, T):
    r, dec = _edge_reader(tmp_cfg)
    K.run_chunk_edges(r, dec, T)
    r.close()


@pytest.mark.parametrize('T', [15, 16, 17])
def test_chunk_edge_cases_in_both_restatements(T):
    """correlate against correlate_brute on the chunk-edge cases.  Reduced: the brute force is a Python loop per product, so it runs
    on (4, 3) over the first 24 and the last 10 rows and on (20, 70) over 2 rows at either end."""
    dec = K.edge_recording()
    for (n_cols, n_out), spans in (((4, 3), ((0, 24), (120, 130))), ((20, 70), ((0, 2), (128, 130)))):
        for before in (0, T):
            for i0, i1 in spans:
                K.edge_case(dec, T, n_cols, n_out, before, i0, i1, brute=True)


@pytest.mark.parametrize('n_cols,n_out,T', K.LIMIT_SHAPES)
def test_limits_on_the_stand_in(tmp_cfg, n_cols, n_out, T):
    r, dec = _make(tmp_cfg)(K.synth_int16(0, K.LIMIT_ROWS, 70, 3), 35)
    K.run_limit(r, dec, n_cols, n_out, T)
    r.close()


def test_tall_templates_on_the_stand_in(tmp_cfg):
    """Reduced: before = 128 only, on 100 rows in chunks of 50 (the chain of 20 x 256 steps runs three times here, and its cost grows
    with the rows)."""
    r, dec = _make(tmp_cfg)(K.synth_int16(0, 100, 70, 3), 50)
    K.run_tall(r, dec, 128, part=(3, 99))
    r.close()


def test_impulse_expectation_is_the_oracles():
    """The literal expectation against the chain.  Reduced: on the 262 rows around the first, the eighth and the last of the 20 impulses
    (the chain over all 5206 rows costs 20 s)."""
    x, k = K.impulse_recording(), K.impulse_templates()
    rows = K.impulse_rows()
    assert len(rows) == K.IMP_COLS and min(np.diff(rows)) > K.IMP_T and rows[0] >= K.IMP_T - 1
    whole = K.impulse_scores()
    assert (whole != 0).sum() == K.IMP_COLS * K.IMP_T * K.IMP_OUT and not np.signbit(whole).any()
    for j in (0, 7, 19):
        i0, i1 = max(0, rows[j] - K.IMP_T - 2), rows[j] + 4
        got = K.scores_of(x, k, 0, i0=i0, i1=i1)
        assert K.impulse_first_mismatch(got, whole[i0:i1], i0) is None
    broken = whole.copy()
    broken[rows[3] - 17, 5] += 1                                    # a mismatch is named by its template entry
    assert K.impulse_first_mismatch(broken, whole)[:2] == (rows[3] - 17, (5, 17, 3))


@pytest.mark.parametrize('kind', ['x', 'k', 'both'])
def test_subnormal_operands_on_the_stand_in(tmp_cfg, kind):
    x, k, cols = K.subnormal_case(kind)
    assert K.is_subnormal(x).all() == (kind != 'k') and K.is_subnormal(k).all() == (kind != 'x')
    assert (np.abs(x) > 1e19).all() == (kind == 'k') and (np.abs(k) > 1e19).all() == (kind == 'x')
    want = K.run_subnormal(_make(tmp_cfg), kind)
    if kind == 'both':                                              # every product underflows: +-0, of both signs
        assert (want == 0).all() and np.signbit(want).any() and not np.signbit(want).all()
    else:                                                           # a flushed operand would give 0 here
        normal = np.isfinite(want) & (np.abs(want) >= K.TINY)
        assert normal.mean() > 0.5
