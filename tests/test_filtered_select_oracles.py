"""The two restatements of mts_filtered_rank_hist in tests/filtered_select_oracle.py held equal -- vectorised (round_add over z) against
the brute count per cell -- in the three key modes, with and without the median reference, on count ranges that cut windows, and on
NaN, +-inf, +-0, denormals and a constant column.  No GPU."""
import numpy as np
import pytest

from mtscomp_amd import hip
from tests.filtered_select_oracle import filtered_round, filtered_round_brute, z_rows, z_rows_brute
from tests.select_oracle import S


def _selectors(z, mode, center, rs):
    """Selector 0 takes every item at the top digit; selector 1 the items under the top digits of one item of each cell, one digit
    down (inactive in a cell now and then)."""
    nw, C = center.shape
    kb = hip.rank_key_bits(np.float32, mode)
    pref = np.zeros((nw, S, C), np.uint64)
    shift = np.zeros((nw, S, C), np.int64)
    shift[:, 0] = kb - 8
    shift[:, 1] = kb - 16
    pick = z[rs.randint(0, z.shape[0], size=(nw, C)), np.arange(C)[None, :]]
    pref[:, 1] = hip.rank_keys(pick, mode, center if mode else None) >> np.uint64(kb - 8)
    shift[:, 1][rs.rand(nw, C) < 0.2] = -1
    return pref, shift


def _same(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


@pytest.mark.parametrize('reference', [0, 1])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_vectorised_equals_brute(mode, reference):
    rs = np.random.RandomState(10 * mode + reference)
    x = rs.randint(-3000, 3000, size=(260, 5)).astype(np.int16)
    x[:, 3] = 7                                                         # a constant column
    vb, ve, x_row0 = 100, 350, 100                                      # the recording is file rows [100, 350) of a buffer from row 100
    for taps in ([1.0], [0.5, -0.25], rs.randn(9)):
        for (rb, re, window, cb, ce) in ((110, 340, 60, 110, 340), (110, 340, 60, 133, 297), (100, 350, 250, 100, 350), (120, 127, 1, 121, 126),
                                         (150, 300, 77, 200, 200)):
            nw = -(-(re - rb) // window)
            center = rs.randn(nw, 5) * 40
            z = z_rows(x, x_row0, vb, ve, rb, re, taps, reference)
            pref, shift = _selectors(z, mode, center, rs)
            cen = center if mode else None
            fast = filtered_round(x, x_row0, vb, ve, taps, reference, rb, re, window, cb, ce, mode, cen, pref, shift)
            slow = filtered_round_brute(x, x_row0, vb, ve, taps, reference, rb, re, window, cb, ce, mode, cen, pref, shift)
            assert _same(fast, slow), (taps, rb, re, window, cb, ce)
            assert int(fast[3].sum()) == ce - cb
            if cb == ce:
                assert not fast[0].any() and (fast[1] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and not fast[2].any()
            elif mode == 0:                                             # selector 0 counts every row of the count range once
                assert (fast[0][:, 0].sum(axis=1) == fast[3][:, None]).all()


@pytest.mark.parametrize('reference', [0, 1])
def test_special_floats(reference):
    rs = np.random.RandomState(3 + reference)
    x = (rs.randn(120, 6) * 10).astype(np.float32)
    x[10, 0] = np.nan
    x[11, 1] = -np.nan
    x[30, 1], x[31, 2] = np.inf, -np.inf
    x[:, 3] = 0
    x[::2, 3] = -0.0
    x[:, 4] = 2.5                                                       # constant
    x[50:60, 5] = np.float32(1e-41) * np.arange(-5, 5, dtype=np.float32)        # denormals
    z = z_rows(x, 0, 0, 120, 0, 120, [1.0], reference)
    assert np.array_equal(z, z_rows_brute(x, 0, 0, 120, 0, 120, [1.0], reference), equal_nan=True)
    if reference:                                                       # a NaN in a row: every column of that row
        assert np.isnan(z[10]).all() and np.isnan(z[11]).all() and not np.isnan(z[12]).any()
    else:
        assert np.array_equal(z, x, equal_nan=True)
    for mode in (0, 1, 2):
        for window in (120, 40):
            nw = 120 // window
            center = rs.randn(nw, 6)
            center[0, 2] = np.nan
            pref, shift = _selectors(np.nan_to_num(z), mode, np.nan_to_num(center), rs)
            cen = center if mode else None
            fast = filtered_round(x, 0, 0, 120, [1.0], reference, 0, 120, window, 5, 118, mode, cen, pref, shift)
            slow = filtered_round_brute(x, 0, 0, 120, [1.0], reference, 0, 120, window, 5, 118, mode, cen, pref, shift)
            assert _same(fast, slow), (mode, window)
            # the NaN key is all ones of key_bits and shows in kmax of the prefix-free selector
            first = z[5:min(window, 118)]                              # window 0 inside the count range
            nan_cell = np.isnan(first).any(axis=0) if not mode else np.isnan(first.astype(np.float64) - center[0]).any(axis=0)
            assert ((fast[2][0, 0] == hip.rank_key_nan(np.float32, mode)) == nan_cell).all()
    # -0 and +0 are one key
    pref = np.zeros((1, S, 6), np.uint64)
    shift = np.full((1, S, 6), 24, np.int64)
    shift[:, 1] = -1
    h, kmin, kmax, _ = filtered_round(x, 0, 0, 120, [1.0], 0, 0, 120, 120, 0, 120, 0, None, pref, shift)
    assert kmin[0, 0, 3] == kmax[0, 0, 3] == 1 << 31 and h[0, 0, 0x80, 3] == 120
