"""The two restatements of mts_localize in tests/localize_oracle.py agree byte for byte: the vectorised one that the suites compare
the device with, and the scalar loops with libm's fmaf.  Small cases with every edge of the definition in them; and the freedom that
the definition leaves a kernel -- taking or skipping the steps whose weight is +0 -- is held to change no bit."""
import numpy as np
import pytest

from mtscomp_amd import api
from mtscomp_amd.synth import synth_int16
from tests.localize_oracle import FILL, MODES, amplitudes, chains, localize, localize_brute, location, reduce_brute, reduce_snippets

FILL_BITS = 0x7fc00000
NEG0 = 0x80000000


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert u.tobytes() == v.tobytes()


def _nan_bits_are_fill(*arrays):
    for a in arrays:
        assert (a.view(np.uint32)[np.isnan(a)] == FILL_BITS).all()


def _positions(n_cols, D, seed=0):
    p = np.random.RandomState(seed).uniform(-50, 50, (n_cols, D)).astype(np.float32)
    p[0] = 0.0
    if n_cols > 2:
        p[2, 0] = -0.0
    return p


@pytest.mark.parametrize('reference', [0, 1])
@pytest.mark.parametrize('dtype', [np.int16, np.float32])
@pytest.mark.parametrize('mode', sorted(MODES.values()))
def test_forms_agree_with_clipping_at_all_four_edges(reference, dtype, mode):
    x = synth_int16(0, 120, 9, 2).astype(dtype)
    taps = api.highpass_taps(300, 5000, 9)
    ev_row = np.array([0, 1, 3, 4, 60, 60, 113, 114, 119, 40])         # before 4, after 6: rows 0 .. 3 and 115 .. 119 clip
    ev_col0 = np.array([-5, -1, 0, 2, 5, 6, 9, -2, 3, 4])              # width 5 over 9 columns: all four edges, some whole events out
    for D in (1, 2, 3, 4):
        pos = _positions(9, D, D)
        got = localize(x, 0, 0, 120, taps, reference, ev_row, ev_col0, 4, 6, 5, mode, pos)
        _same(got, localize_brute(x, 0, 0, 120, taps, reference, ev_row, ev_col0, 4, 6, 5, mode, pos))
        amp, weight, moment, best = got
        assert amp.shape == (10, 5) and weight.shape == (10,) and moment.shape == (10, D) and best.dtype == np.int64
        nan = np.isnan(amp)
        # an event whose positions all lie outside: NaN amplitudes, weight and moment +0, no best
        for e in (0, 6):
            assert nan[e].all() and weight[e].view(np.uint32) == 0 and not moment[e].view(np.uint32).any() and best[e] == -1
        # a clipped event keeps the amplitudes of the rows and positions it has (waveforms' extrema rule)
        assert nan[1, 0] and not nan[1, 1:].any() and not nan[8].any() and not nan[2].any()
        assert not nan[4, :4].any() and nan[4, 4]                        # position 9 of 9 columns
        assert (best[[1, 2, 3, 4, 5, 7, 8, 9]] >= 0).all()
        _nan_bits_are_fill(amp, weight, moment)


def _special_wave():
    inf, nan, tiny = np.float32(np.inf), np.float32(np.nan), np.float32(1e-42)
    # (T = 4, W = 10), one event; columns: plain | +inf and -inf | all NaN | -0 then +0 | +0 then -0 | a plateau of minima and maxima |
    # a denormal | overflow of hi - lo | all negative | one entry and NaNs
    cols = [[1.0, -2.0, 3.0, 0.5], [inf, 1.0, -inf, 2.0], [nan, nan, nan, nan], [-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, 0.0, -0.0],
            [-3.0, 2.0, -3.0, 2.0], [tiny, -tiny, 0.0, tiny], [3e38, -3e38, 1.0, 2.0], [-1.0, -4.0, -2.0, -1.0], [nan, nan, 7.0, nan]]
    return np.array(cols, np.float32).T.copy()[None]


def test_forms_agree_on_special_values_in_every_mode():
    wave = _special_wave()
    assert wave.shape == (1, 4, 10)
    pos = _positions(12, 2, 1)
    inf = np.float32(np.inf)
    for mode in range(4):
        for col0 in (0, 2, -3):
            got = reduce_snippets(wave, np.array([col0]), pos, mode)
            _same(got, reduce_brute(wave, np.array([col0]), pos, mode))
            _nan_bits_are_fill(got[0], got[1], got[2])
    a = {name: amplitudes(wave, m)[0] for name, m in MODES.items()}
    assert a['ptp'][0] == 5.0 and a['neg'][0] == 2.0 and a['pos'][0] == 3.0 and a['abs'][0] == 3.0
    assert a['ptp'][1] == inf and a['neg'][1] == inf and a['pos'][1] == inf and a['abs'][1] == inf
    for name in MODES:
        assert a[name].view(np.uint32)[2] == FILL_BITS                   # a column that is NaN throughout
    # -0 == +0: the first wins, with its own bits; 'neg' negates exactly (+0 gives -0)
    assert a['pos'].view(np.uint32)[3] == NEG0 and a['pos'].view(np.uint32)[4] == 0
    assert a['neg'].view(np.uint32)[3] == 0 and a['neg'].view(np.uint32)[4] == NEG0
    assert a['abs'].view(np.uint32)[3] == 0 and a['abs'].view(np.uint32)[4] == 0
    assert a['ptp'].view(np.uint32)[3] == 0 and a['ptp'].view(np.uint32)[4] == 0           # (-0) - (-0) = +0 and (+0) - (+0) = +0
    assert a['ptp'][5] == 5.0 and a['neg'][5] == 3.0 and a['pos'][5] == 2.0
    assert 0 < a['ptp'][6] < np.finfo(np.float32).tiny                   # a denormal amplitude is kept
    assert a['ptp'][7] == inf and a['pos'][7] == np.float32(3e38)        # hi - lo overflows
    assert a['pos'][8] == -1.0 and a['neg'][8] == 4.0 and a['ptp'][8] == 3.0
    assert (a['ptp'][9], a['neg'][9], a['pos'][9], a['abs'][9]) == (0.0, -7.0, 7.0, 7.0)   # NaN entries are skipped
    # an amplitude of +inf: weight inf, and inf * 0 (position 0 is the origin) makes the moment NaN, in the fill's bits
    _, weight, moment, best = reduce_snippets(wave, np.array([-1]), pos, MODES['ptp'])      # column 1 (the +inf one) sits on position 0
    assert weight[0] == inf and (moment.view(np.uint32) == FILL_BITS).all() and best[0] == 1
    _, weight, moment, best = reduce_snippets(wave, np.array([1]), pos, MODES['ptp'])
    assert weight[0] == inf and not np.isfinite(moment).any() and best[0] == 1               # the first of the two +inf amplitudes


def test_negative_amplitudes_weigh_nothing_and_best_ignores_nan():
    wave = _special_wave()[:, :, [8, 2, 8]]                            # all negative | all NaN | all negative
    pos = _positions(3, 3, 2)
    amp, weight, moment, best = reduce_snippets(wave, np.array([0]), pos, MODES['pos'])
    _same((amp, weight, moment, best), reduce_brute(wave, np.array([0]), pos, MODES['pos']))
    assert amp[0, 0] == -1.0 and np.isnan(amp[0, 1]) and amp[0, 2] == -1.0
    assert weight.view(np.uint32)[0] == 0 and not moment.view(np.uint32).any()             # +0, never -0
    assert best[0] == 0                                                  # the first of equal amplitudes, the NaN between them ignored
    assert location(moment, weight).view(np.uint32).tolist() == [[FILL_BITS] * 3]
    # -inf is an amplitude like another: it beats nothing but is a best when alone
    one = np.full((1, 2, 3), FILL, np.float32)
    one[0, 0, 1] = -np.inf
    amp, weight, moment, best = reduce_snippets(one, np.array([0]), pos, MODES['pos'])
    _same((amp, weight, moment, best), reduce_brute(one, np.array([0]), pos, MODES['pos']))
    assert best[0] == 1 and weight.view(np.uint32)[0] == 0


def test_ties_for_best_take_the_lowest_position():
    wave = np.zeros((2, 3, 6), np.float32)
    wave[0, 1, [1, 3, 4]] = -5.0                                         # three equal troughs
    wave[1, 0, 2], wave[1, 2, 5] = -0.0, 0.0
    pos = _positions(6, 1, 3)
    for mode, want in ((MODES['neg'], [1, 0]), (MODES['ptp'], [1, 0]), (MODES['abs'], [1, 0]), (MODES['pos'], [0, 0])):
        got = reduce_snippets(wave, np.array([0, 0]), pos, mode)
        _same(got, reduce_brute(wave, np.array([0, 0]), pos, mode))
        assert got[3].tolist() == want


@pytest.mark.parametrize('T,W,D', [(1, 1, 1), (1, 7, 4), (9, 1, 2), (2, 33, 3)])
def test_forms_agree_on_small_shapes(T, W, D):
    rs = np.random.RandomState(T * 100 + W + D)
    wave = rs.standard_normal((8, T, W)).astype(np.float32)
    wave[rs.rand(8, T, W) < 0.2] = FILL
    pos = _positions(W + 4, D, 4)
    col0 = rs.randint(-W, W + 4, 8)
    for mode in range(4):
        _same(reduce_snippets(wave, col0, pos, mode), reduce_brute(wave, col0, pos, mode))


def test_skipping_zero_weight_steps_changes_no_bit():
    rs = np.random.RandomState(11)
    wave = rs.standard_normal((40, 5, 12)).astype(np.float32)
    wave[rs.rand(40, 5, 12) < 0.3] = FILL
    wave[3], wave[4, :, :6] = 0.0, -0.0                                  # zero amplitudes, of both signs under 'neg' and 'pos'
    wave[5, 2, 3], wave[6, 1, 0], wave[7, 0, 11] = np.inf, -np.inf, 3e38
    wave[7, 1, 11] = -3e38
    pos = _positions(16, 4, 5)
    pos[1], pos[5, 2] = -0.0, -0.0                                       # a g = +0 step against -0: +0 * -0 = -0, and +0 + -0 = +0
    col0 = rs.randint(-12, 16, 40)
    col0[:8] = 0
    zero_steps = 0
    for mode in range(4):
        a = amplitudes(wave, mode)
        zero_steps += int((~(a > 0)).sum())
        taken, skipped = chains(a, col0, pos), chains(a, col0, pos, skip_zero=True)
        _same(taken, skipped)
        assert not (taken[0].view(np.uint32) == NEG0).any() and not (taken[1].view(np.uint32) == NEG0).any()   # an accumulator is never -0
        assert np.isinf(taken[0]).any()                                  # (a zero step leaves an inf, and the NaN it makes, what they are)
    assert zero_steps > 100


def test_location_is_the_host_quotient():
    moment = np.array([[6.0, -3.0], [0.0, 0.0], [1.0, np.inf], [np.inf, 1.0], [FILL, 2.0], [1.0, 1.0]], np.float32)
    weight = np.array([3.0, 0.0, np.inf, np.inf, 1.0, FILL], np.float32)
    loc = location(moment, weight)
    assert loc.dtype == np.float32 and loc[0].tolist() == [2.0, -1.0]
    bits = loc.view(np.uint32)
    assert (bits[1] == FILL_BITS).all()                                  # weight 0
    assert loc[2, 0] == 0.0 and bits[2, 1] == FILL_BITS and bits[3, 0] == FILL_BITS and loc[3, 1] == 0.0      # inf / inf
    assert bits[4, 0] == FILL_BITS and loc[4, 1] == 2.0 and (bits[5] == FILL_BITS).all()
    third = location(np.array([[1.0]], np.float32), np.array([3.0], np.float32))
    assert third[0, 0] == np.float32(1.0 / 3.0)                          # one rounding of the float64 quotient
