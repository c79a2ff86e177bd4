"""The two restatements of mts_waveforms (tests/waveforms_oracle.py) against each other: the vectorised one, which every other test
leans on, equals the brute-force one on the edges of the definition."""
import numpy as np
import pytest

from mtscomp_amd import api
from mtscomp_amd.synth import synth_int16
from tests.detect_oracle import detect_events
from tests.waveforms_oracle import BASE_COUNTS, FILL, edge_counts, extrema, waveforms, waveforms_brute


def _same(got, want):
    for g, w, name in zip(got, want, ('wave', 'min', 'argmin', 'max', 'argmax')):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name


def test_fill_is_the_quiet_nan():
    assert FILL.tobytes() == np.uint32(0x7fc00000).tobytes() and FILL.dtype == np.float32


@pytest.mark.parametrize('reference', [0, 1])
def test_base_case_counts_and_brute_force(reference):
    x = synth_int16(0, 3000, 70, 4)
    taps = api.highpass_taps(300, 5000, 65)
    row, pos, amp = detect_events(x, 0, 0, 3000, 0, 3000, taps, 12, 0, reference, 7, 3)
    col0 = pos - 8
    assert edge_counts(row, col0, 20, 41, 17, 3000, 70) == BASE_COUNTS[reference]
    got = waveforms(x, 0, 0, 3000, taps, reference, row, col0, 20, 41, 17)
    assert got[0][np.arange(row.size), 20, 8].tobytes() == amp.tobytes()        # the centre sample is detect's amplitude
    # the brute force on the events at the edges and every 7th of the others
    pick = np.nonzero((row < 20) | (row + 41 > 3000) | (col0 < 0) | (col0 + 17 > 70) | (np.arange(row.size) % 7 == 0))[0]
    want = waveforms_brute(x, 0, 0, 3000, taps, reference, row[pick], col0[pick], 20, 41, 17)
    _same([g[pick] for g in got], want)


@pytest.mark.parametrize('before,after,width', [(5, 9, 5), (0, 1, 1), (1, 0, 3), (0, 3, 12), (40, 40, 2)])
@pytest.mark.parametrize('reference', [0, 1])
def test_shapes_edges_and_any_order(before, after, width, reference):
    rs = np.random.RandomState(before * 100 + after)
    x = (rs.randn(60, 7) * 50).astype(np.float32)
    taps = rs.randn(5)
    ev_row = np.concatenate(([10, 59, 59, 30, 10], rs.randint(10, 60, 30)))      # the file rows of x are [10, 70), the recording [10, 60)
    ev_col0 = rs.randint(-width - 1, 8, ev_row.size)
    got = waveforms(x, 10, 10, 60, taps, reference, ev_row, ev_col0, before, after, width)
    _same(got, waveforms_brute(x, 10, 10, 60, taps, reference, ev_row, ev_col0, before, after, width))
    assert (got[2] == -1).any() == bool((np.isnan(got[1])).any())


def test_extrema_special_values():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    wave = np.array([[[nan, 0.0, -0.0], [-0.0, 0.0, nan]],                       # zeros of both signs: the first, with its own bits
                     [[nan, nan, nan], [nan, nan, nan]],                         # nothing
                     [[nan, inf, inf], [inf, nan, inf]],                         # the stand-in of the vectorised reduction itself
                     [[nan, -inf, -inf], [-inf, nan, -inf]],
                     [[3.0, 1.0, 1.0], [7.0, 7.0, -inf]],
                     [[nan, nan, nan], [nan, nan, 5.0]]], np.float32)
    vmin, amin, vmax, amax = extrema(wave)
    assert amin.tolist() == [1, -1, 1, 1, 5, 5] and amax.tolist() == [1, -1, 1, 1, 3, 5]
    assert vmin[0].tobytes() == np.float32(0.0).tobytes() and vmax[0].tobytes() == np.float32(0.0).tobytes()
    assert vmin[1].tobytes() == vmax[1].tobytes() == FILL.tobytes()
    assert (vmin[2], vmax[2], vmin[3], vmax[3]) == (inf, inf, -inf, -inf)
    assert (vmin[4], vmax[4], vmin[5], vmax[5]) == (-inf, 7.0, 5.0, 5.0)
    wave[0, 0, 1], wave[0, 1, 0] = -0.0, 0.0
    vmin, amin, vmax, amax = extrema(wave)
    assert amin[0] == amax[0] == 1 and vmin[0].tobytes() == vmax[0].tobytes() == np.float32(-0.0).tobytes()


def test_special_values_through_the_definition():
    rs = np.random.RandomState(5)
    x = (rs.randn(200, 9) * 10).astype(np.float32)
    x[50, 1], x[90, 2], x[120, 3] = np.nan, np.inf, -np.inf
    x[150:153] = 0.0
    x[151, 4] = -0.0
    ev_row = np.array([48, 50, 52, 88, 90, 119, 121, 150, 151, 152, 10, 199, 0])
    ev_col0 = np.array([0, 1, -1, 1, 2, 3, 0, 3, 4, 2, 5, 7, -2])
    for reference in (0, 1):
        for taps in ([1.0], [0.25, 0.5, 0.25]):
            got = waveforms(x, 0, 0, 200, taps, reference, ev_row, ev_col0, 2, 3, 3)
            _same(got, waveforms_brute(x, 0, 0, 200, taps, reference, ev_row, ev_col0, 2, 3, 3))
