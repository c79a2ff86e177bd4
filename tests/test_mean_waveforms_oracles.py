"""The two restatements of mts_mean_waveforms (tests/mean_waveforms_oracle.py) against each other: the vectorised one, which every
other test leans on, equals the brute-force one on the edges of the definition -- and the inputs reach those edges."""
import numpy as np
import pytest

from mtscomp_amd import api
from mtscomp_amd.synth import synth_int16
from tests.detect_oracle import detect_events
from tests.mean_waveforms_oracle import mean_of, mean_waveforms, mean_waveforms_brute, rint_half_even
from tests.waveforms_oracle import BASE_COUNTS, edge_counts


def _same(got, want):
    for g, w, name, t in zip(got, want, ('sum', 'count', 'skipped'), (np.int64, np.int32, np.int64)):
        assert g.dtype == w.dtype == t and g.shape == w.shape and g.tobytes() == w.tobytes(), name


def test_rint_half_even_is_numpys():
    for d in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, 2.0 ** 41 + 0.5, -(2.0 ** 41) - 1.5, 7.0, -7.25, 2.0 ** 42 - 0.5):
        assert rint_half_even(d) == int(np.rint(d)), d


@pytest.mark.parametrize('reference', [0, 1])
def test_base_case_reaches_every_edge_and_equals_brute_force(reference):
    x = synth_int16(0, 3000, 70, 4)
    taps = api.highpass_taps(300, 5000, 65)
    row, pos, _ = detect_events(x, 0, 0, 3000, 0, 3000, taps, 12, 0, reference, 7, 3)
    col0 = pos - 8
    counts = edge_counts(row, col0, 20, 41, 17, 3000, 70)
    assert counts == BASE_COUNTS[reference]
    assert min(counts[k] for k in ('clip_lo', 'clip_hi', 'clip_left', 'clip_right')) > 0       # clipped at both ends and both column edges
    label = pos % 5 + (pos % 5 >= 3)                                     # labels 0, 1, 2, 4, 5 of 7: 3 and 6 have no event
    got = mean_waveforms(x, 0, 0, 3000, taps, reference, row, col0, label, 7, 20, 41, 17, 2.0 ** -16)
    total, count, skipped = got
    events = np.bincount(label, minlength=7)
    assert (events[[3, 6]] == 0).all() and (events[[0, 1, 2, 4, 5]] > 0).all()
    assert not total[[3, 6]].any() and not count[[3, 6]].any() and not skipped.any()
    assert (count.max(axis=(1, 2)) == events).all()                      # some entry of every label is clipped for no event ...
    assert (count.min(axis=(1, 2)) < events)[events > 0].all()           # ... and some entry for at least one
    assert int(count.sum()) == int(((row[:, None] - 20 + np.arange(61) >= 0) & (row[:, None] - 20 + np.arange(61) < 3000)).sum(axis=1)
                                   @ ((col0[:, None] + np.arange(17) >= 0) & (col0[:, None] + np.arange(17) < 70)).sum(axis=1))
    # the brute force on the events at the edges and every 7th of the others
    pick = np.nonzero((row < 20) | (row + 41 > 3000) | (col0 < 0) | (col0 + 17 > 70) | (np.arange(row.size) % 7 == 0))[0]
    _same(mean_waveforms(x, 0, 0, 3000, taps, reference, row[pick], col0[pick], label[pick], 7, 20, 41, 17, 2.0 ** -16),
          mean_waveforms_brute(x, 0, 0, 3000, taps, reference, row[pick], col0[pick], label[pick], 7, 20, 41, 17, 2.0 ** -16))
    mean = mean_of(total, count, 2.0 ** -16)
    assert mean.dtype == np.float32 and np.array_equal(np.isnan(mean), count == 0)
    assert set(mean[count == 0].view(np.uint32).tolist()) == {0x7fc00000}


@pytest.mark.parametrize('before,after,width', [(5, 9, 5), (0, 1, 1), (1, 0, 3), (0, 3, 12), (40, 40, 2)])
@pytest.mark.parametrize('reference', [0, 1])
def test_shapes_edges_any_order_and_resolutions(before, after, width, reference):
    rs = np.random.RandomState(before * 100 + after)
    x = (rs.randn(60, 7) * 50).astype(np.float32)
    taps = rs.randn(5)
    ev_row = np.concatenate(([10, 59, 59, 30, 10], rs.randint(10, 60, 30)))      # the file rows of x are [10, 70), the recording [10, 60)
    ev_col0 = rs.randint(-width - 1, 8, ev_row.size)
    label = rs.randint(0, 4, ev_row.size)
    for resolution in (2.0 ** -16, 1.0, 2.0 ** 3, 2.0 ** -60, 2.0 ** 60):
        got = mean_waveforms(x, 10, 10, 60, taps, reference, ev_row, ev_col0, label, 5, before, after, width, resolution)
        _same(got, mean_waveforms_brute(x, 10, 10, 60, taps, reference, ev_row, ev_col0, label, 5, before, after, width, resolution))
        if resolution == 2.0 ** -60:
            assert got[2].sum() > 0 and not got[1].all()                 # 50 * 2^60 >= 2^42: nearly everything is skipped
        if resolution == 2.0 ** 60:
            assert not got[0].any() and got[1].any()                     # everything rounds to 0 and is counted
    order = rs.permutation(ev_row.size)
    a = mean_waveforms(x, 10, 10, 60, taps, reference, ev_row, ev_col0, label, 5, before, after, width, 0.5)
    _same(mean_waveforms(x, 10, 10, 60, taps, reference, ev_row[order], ev_col0[order], label[order], 5, before, after, width, 0.5), a)


def test_skips_ties_and_the_limit():
    x = np.zeros((40, 3), np.float32)
    x[:, 0] = np.arange(-20, 20)                                         # with resolution 2: every odd value is a tie
    x[5, 1], x[6, 1], x[7, 1], x[8, 1] = np.nan, np.inf, -np.inf, np.float32(2.0 ** 43)         # = 2^42 * resolution: skipped
    x[9, 1] = np.nextafter(np.float32(2.0 ** 43), np.float32(0))         # just under: counted
    x[10, 1] = -np.float32(2.0 ** 43)
    ev_row = np.arange(40)
    got = mean_waveforms(x, 0, 0, 40, [1.0], 0, ev_row, np.zeros(40, int), ev_row % 2, 2, 0, 1, 3, 2.0)
    _same(got, mean_waveforms_brute(x, 0, 0, 40, [1.0], 0, ev_row, np.zeros(40, int), ev_row % 2, 2, 0, 1, 3, 2.0))
    total, count, skipped = got
    assert skipped.tolist() == [3, 2] and count[:, 0, 1].tolist() == [17, 18] and count[:, 0, 0].tolist() == [20, 20]
    assert total[1, 0, 1] == int(x[9, 1]) // 2
    # half to even, both signs and both parities: -19/2 -> -10, -17/2 -> -8, 1/2 -> 0, 3/2 -> 2
    odd = np.arange(-19, 20, 2)
    want = np.array([rint_half_even(v / 2.0) for v in odd])
    assert {int(v) for v in want[odd < 0] % 2} == {0} and (-10 in want) and (-8 in want) and (0 in want) and (2 in want)
    assert total[1, 0, 0] == want.sum() and total[0, 0, 0] == np.arange(-20, 20, 2).sum() // 2
