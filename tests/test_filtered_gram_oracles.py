"""The two restatements of mts_filtered_gram in tests/filtered_gram_oracle.py against each other: gram_partials of z_rows (float64 BLAS
per group: what the lane codec of the CPU suite returns) and the brute form (the median of every row by sorting in Python, the Gram
row by row in np.longdouble).  They are held equal within gram_oracle.gram_bound: a BLAS sum over n rows rounds a product at most n
times whatever its order, so h = n; the longdouble form's own error is (n + 2) * 2^-64 * sum |z_i z_j|.  NaN entries sit at the same
places.  No GPU."""
import numpy as np
import pytest

from mtscomp_amd import api, hip
from tests.filtered_gram_oracle import call_rows, filtered_partials, filtered_partials_brute
from tests.filtered_select_oracle import z_rows, z_rows_brute
from tests.gram_oracle import UL, gamma, gram_bound

HP = api.highpass_taps(300, 30000, 21)


def _recording(rows, nc, seed, dtype='int16'):
    rs = np.random.RandomState(seed)
    x = rs.randn(rows, nc) * 300 + rs.randn(nc) * 1000 + 500 * np.sin(np.arange(rows) / 40.)[:, None]
    return x.astype(dtype)


def _hold_equal(x, vb, ve, taps, reference, rb, re, window, g0, g1):
    G, S = filtered_partials(x, 0, vb, ve, taps, reference, rb, re, window, g0, g1)
    Gb, Sb, A, rows = filtered_partials_brute(x, 0, vb, ve, taps, reference, rb, re, window, g0, g1)
    assert G.dtype == np.float64 and S.dtype == np.float64 and G.shape == Gb.shape and S.shape == Sb.shape
    assert np.array_equal(np.isnan(G), np.isnan(Gb.astype(np.float64))) and np.array_equal(np.isnan(S), np.isnan(Sb.astype(np.float64)))
    for j in range(g1 - g0):
        n = int(rows[j])
        lo, hi = hip.gram_group_rows(rb, re, window, g0 + j)
        with np.errstate(invalid='ignore', over='ignore'):
            fin = np.isfinite(A[j])
            allow = gram_bound(n, A[j], n) + (n + 2) * UL * A[j]
            err = np.abs(G[j].astype(np.longdouble) - Gb[j])
            sabs = np.abs(z_rows(x, 0, vb, ve, lo, hi, taps, reference).astype(np.float64)).sum(axis=0)
            serr = np.abs(S[j].astype(np.longdouble) - Sb[j])
        assert np.where(fin, err <= allow, True).all()
        assert np.where(np.isfinite(sabs), serr <= (gamma(n + 1) + (n + 2) * UL) * sabs, True).all()
    return G, S


@pytest.mark.parametrize('reference', [0, 1])
@pytest.mark.parametrize('nc', [1, 4, 5])
def test_two_forms_agree(reference, nc):
    x = _recording(700, nc, seed=3 + nc)
    for taps in ([1.0], [0.5, 0.25, -0.75], HP):
        for rb, re, window in ((0, 700, 700), (0, 700, 256), (13, 650, 100), (300, 301, 1)):
            n_groups = hip.gram_groups(rb, re, window)
            G, _ = _hold_equal(x, 0, 700, taps, reference, rb, re, window, 0, n_groups)
            # a run of groups in the middle is the same partials
            if n_groups > 2:
                Gm, _ = filtered_partials(x, 0, 0, 700, taps, reference, rb, re, window, 1, n_groups - 1)
                assert Gm.tobytes() == G[1:-1].tobytes()


def test_valid_range_and_offset_chunks():
    """x = 0 outside [vb, ve); x given from a row other than 0."""
    x = _recording(500, 3, seed=9)
    full, _ = filtered_partials(x, 0, 100, 400, HP, 1, 100, 400, 128, 0, 3)
    G, S = filtered_partials(x[90:420], 90, 100, 400, HP, 1, 100, 400, 128, 0, 3)
    assert G.tobytes() == full.tobytes()
    Gb, _, A, _ = filtered_partials_brute(x[90:420], 90, 100, 400, HP, 1, 100, 400, 128, 0, 3)
    assert (np.abs(G.astype(np.longdouble) - Gb) <= gram_bound(128, A, 128) + 130 * UL * A).all()
    zeroed = x.copy()
    zeroed[:100] = 0
    zeroed[400:] = 0
    assert filtered_partials(zeroed, 0, 0, 500, HP, 1, 100, 400, 128, 0, 3)[0].tobytes() == full.tobytes()
    assert call_rows(100, 400, 128, 1, 3) == (228, 400)


def test_nan_rows():
    """A NaN item: its column's entries without a reference, every entry of the window with the median reference."""
    x = _recording(300, 4, seed=11, dtype='float32')
    x[120, 2] = np.nan
    x[200, 1] = np.inf
    assert z_rows(x, 0, 0, 300, 100, 140, [1.0], 1).tobytes() == z_rows_brute(x, 0, 0, 300, 100, 140, [1.0], 1).tobytes()
    G, S = _hold_equal(x, 0, 300, [1.0], 0, 0, 300, 150, 0, 2)
    assert np.isnan(G[0][2]).all() and np.isnan(G[0][:, 2]).all() and np.isfinite(G[0][[0, 1, 3]][:, [0, 1, 3]]).all()
    assert np.isnan(S[0, 2]) and np.isposinf(S[1, 1]) and np.isposinf(G[1, 1, 1])
    G, S = _hold_equal(x, 0, 300, [1.0], 1, 0, 300, 150, 0, 2)
    assert np.isnan(G[0]).all() and np.isnan(S[0]).all() and np.isposinf(G[1, 1, 1]) and np.isfinite(G[1, 0, 0])
