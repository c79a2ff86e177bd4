"""The two numpy restatements of mts_match_templates (tests/tmatch_oracle.py) agree with each other -- the row-maximum form the
kernels use against the plain loop over every (t', k') -- on random data, tied templates, a constant recording, NaN and inf, and
hold the consequences the definition names."""
import numpy as np
import pytest

from mtscomp_amd.synth import synth_int16
from tests.correlate_oracle import correlate
from tests.tmatch_oracle import events_of_scores, events_of_scores_brute, match_templates, match_templates_brute

EXCLUDES = (0, 1, 2, 20, 255)


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _both(score, a, i0, i1, thr, R):
    fast, slow = events_of_scores(score, a, i0, i1, thr, R), events_of_scores_brute(score, a, i0, i1, thr, R)
    assert _same(fast, slow)
    return fast


@pytest.mark.parametrize('R', EXCLUDES)
def test_random_scores_and_ties(R):
    rs = np.random.RandomState(R)
    score = rs.randn(300, 5).astype(np.float32)
    thr = np.percentile(score, 60, axis=0).astype(np.float32)
    n0 = _both(score, 0, 0, 300, thr, 0)[0].size
    n = _both(score, 0, 0, 300, thr, R)[0].size
    assert n0 > 0 and n > 0 and (R == 0 or n < n0)
    coarse = np.round(score * 2) / 2                                      # many exact ties, within rows and between them
    coarse[:, 3] = coarse[:, 1]
    coarse[:, 4] = coarse[:, 0]
    row, tpl, _ = _both(coarse.astype(np.float32), 0, 0, 300, -10.0, R)
    assert row.size and not np.isin(tpl, (3, 4)).any()                    # of identical templates the lower index has the event
    assert (np.diff(row) > R).all()                                       # at most one event per neighbourhood
    _both(score, 40, 100, 220, thr, R)                                    # a slab that begins past row 0: rows before it do not exist


@pytest.mark.parametrize('R', EXCLUDES)
def test_special_values(R):
    rs = np.random.RandomState(7)
    score = rs.randn(120, 4).astype(np.float32)
    score[10] = np.nan                                                    # a row of NaNs: no event, beats nothing
    score[30, 1] = np.nan
    score[50, 2] = np.inf
    score[52, 0] = np.inf                                                 # two equal +inf: the earlier wins
    score[70] = -np.inf
    score[90, 0], score[90, 1] = -0.0, 0.0
    row, tpl, val = _both(score, 0, 0, 120, -3e38, R)
    assert 10 not in row and 50 in row and tpl[list(row).index(50)] == 2 and np.isposinf(val[list(row).index(50)])
    assert (52 in row) == (R < 2)
    assert not np.isnan(val).any()
    zeros = np.zeros((40, 3), np.float32)
    zeros[::2, 1] = -0.0                                                  # -0 equals +0: one plateau
    row, tpl, val = _both(zeros, 0, 0, 40, -1.0, R)
    assert row.tolist() == (list(range(40)) if R == 0 else [0]) and not tpl.any() and val.tobytes() == zeros[row, 0].tobytes()
    assert _both(zeros, 0, 0, 40, 0.0, R)[0].size == 0                    # a threshold is exceeded, not met


def test_plateau_gives_its_first_row():
    for R in (1, 2, 20, 255):
        zeros = np.zeros((600, 2), np.float32)
        assert _both(zeros, 0, 0, 600, -1.0, R)[0].tolist() == [0]       # every later row has an equal earlier neighbour
        ramp = np.arange(600, dtype=np.float32)[:, None] * np.ones((1, 2), np.float32)
        assert _both(ramp, 0, 0, 600, -1.0, R)[0].tolist() == [599]
        assert _both(-ramp, 0, 0, 600, -1e9, R)[0].tolist() == [0]


@pytest.mark.parametrize('R', EXCLUDES)
def test_on_recordings_and_stitch(R):
    x = synth_int16(0, 300, 6, 5)
    rs = np.random.RandomState(3)
    k = rs.randn(5, 7, 6).astype(np.float32)
    k[4] = k[0]
    k[3] = k[1]
    taps = rs.randn(9)
    thr = np.percentile(correlate(x, 0, 0, 300, 0, 300, taps, 1, 3, k), 90, axis=0).astype(np.float32)
    args = (taps, 1, 3, k, thr, R)
    whole = match_templates(x, 0, 0, 300, 0, 300, *args)
    assert _same(whole, match_templates_brute(x, 0, 0, 300, 0, 300, *args))
    assert whole[0].size and not np.isin(whole[1], (3, 4)).any()
    score = correlate(x, 0, 0, 300, 0, 300, taps, 1, 3, k)
    assert whole[2].tobytes() == score[whole[0], whole[1]].tobytes()
    for a, b, c in ((0, 100, 300), (0, 1, 2), (120, 121, 300), (37, 299, 300)):
        left, right = match_templates(x, 0, 0, 300, a, b, *args), match_templates(x, 0, 0, 300, b, c, *args)
        assert _same([np.concatenate(p) for p in zip(left, right)], match_templates(x, 0, 0, 300, a, c, *args))
        assert _same(left, match_templates_brute(x, 0, 0, 300, a, b, *args))
    # a constant recording, no filter, an all-ones template: one event, at the first full-window row
    const = np.full((200, 3), 7, np.int16)
    ones = np.ones((1, 5, 3), np.float32)
    got = match_templates(const, 0, 0, 200, 0, 200, [1.0], 0, 2, ones, 1.0, R)
    assert _same(got, match_templates_brute(const, 0, 0, 200, 0, 200, [1.0], 0, 2, ones, 1.0, R))
    if R:
        assert got[0].tolist() == [2]
    # rows that read nothing of the recording score +0: an event under a negative threshold, none under a positive one
    top = match_templates(const[:0], 0, 0, 200, 0, 1, [1.0], 0, 5, ones, -1.0, 0)
    assert (top[0].tolist(), top[1].tolist(), top[2].tobytes()) == ([0], [0], np.zeros(1, np.float32).tobytes())
    assert match_templates(const[:0], 0, 0, 200, 0, 1, [1.0], 0, 5, ones, 1.0, 0)[0].size == 0
