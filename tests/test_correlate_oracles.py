"""The numpy restatements of mts_correlate (tests/correlate_oracle.py) against each other and against what the definition implies:
the vectorised chain and the brute-force one agree byte for byte, the chain is a matched filter (a float64 einsum, a one-hot
template) and its T = 1 case is mts_project's chain."""
import numpy as np
import pytest

from tests.correlate_oracle import FILL, correlate, correlate_brute, correlate_chain, reference_rows
from tests.project_oracle import project_chain_f32

# (rows, columns, T, K): the shapes the vectorised chain was timed on (about 2 s each)
SHAPES = [(600, 70, 61, 17), (200, 385, 61, 3), (300, 65, 256, 5)]


@pytest.mark.parametrize('n_cols,T,before,K,taps,reference', [
    (1, 1, 0, 1, [1.0], 0), (3, 2, 2, 2, [1.0], 0), (4, 3, 1, 3, [0.25, 0.5, 0.25], 1), (5, 5, 0, 2, [1.0, -1.0], 1), (9, 4, 4, 1, [0.5], 0)])
def test_two_restatements_agree(n_cols, T, before, K, taps, reference):
    rs = np.random.RandomState(n_cols * 31 + T)
    x = rs.randint(-300, 300, size=(40, n_cols)).astype(np.int16)
    k = rs.randn(K, T, n_cols)
    k[0, 0, 0] = 0.0
    for i0, i1 in ((0, 9), (33, 40), (17, 23)):                        # both ends of the recording: the rows outside are +0
        a = correlate(x, 0, 0, 40, i0, i1, taps, reference, before, k)
        b = correlate_brute(x, 0, 0, 40, i0, i1, taps, reference, before, k)
        assert a.dtype == b.dtype == np.float32 and a.shape == (i1 - i0, K)
        assert a.tobytes() == b.tobytes()


def test_special_values_agree_and_nan_is_canonical():
    x = np.random.RandomState(2).randn(30, 5).astype(np.float32)
    x[7, 1], x[12, 2], x[13, 2], x[20, 0], x[21] = np.nan, np.inf, -np.inf, -0.0, 1e-30
    k = np.random.RandomState(3).randn(3, 4, 5)
    k[1] = 0.0                                                          # inf * 0 is NaN: zero entries are not skipped
    k[2] *= 1e-12                                                       # products in the subnormal range
    a = correlate(x, 0, 0, 30, 0, 30, [1.0], 0, 1, k)
    b = correlate_brute(x, 0, 0, 30, 0, 30, [1.0], 0, 1, k)
    assert a.tobytes() == b.tobytes()
    nan = np.isnan(a)
    assert nan[:, 1].sum() >= 8 and set(a[nan].view(np.uint32).tolist()) == {0x7fc00000} and np.isnan(FILL)
    assert np.isinf(a[:, 0]).any()


@pytest.mark.parametrize('rows,n_cols,T,K', SHAPES)
def test_chain_is_a_matched_filter(rows, n_cols, T, K):
    rs = np.random.RandomState(rows)
    z = rs.randn(rows + T - 1, n_cols).astype(np.float32)
    k = rs.randn(K, T, n_cols).astype(np.float32)
    got = correlate_chain(z, k)
    win = np.lib.stride_tricks.sliding_window_view(z.astype(np.float64), T, axis=0)      # (rows, n_cols, T)
    want = np.einsum('ijt,ktj->ik', win, k.astype(np.float64))
    scale = np.einsum('ijt,ktj->ik', np.abs(win), np.abs(k.astype(np.float64)))
    # "relative" is the largest error against the largest score, max |chain - einsum| / max |einsum|: measured 2.3e-6, 4.8e-6 and
    # 5.6e-6 on the three shapes with these seeds.  (Element by element the ratio is unbounded: scores near zero are sums that cancel
    # -- 9e-3 at worst here -- so that quantity is held to the chain's own bound below instead.)
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print('max |chain - einsum| / max |einsum| = %.3g' % rel)
    assert rel < 1e-5
    # a float32 chain of n terms errs by at most gamma_n of the sum of magnitudes, element by element
    n = T * (-(-n_cols // 4) * 4)
    assert float((np.abs(got - want) / scale).max()) <= n * 2.0 ** -24 / (1 - n * 2.0 ** -24)


def test_one_hot_template_reads_z():
    rs = np.random.RandomState(5)
    x = rs.randint(-2000, 2000, size=(120, 7)).astype(np.int16)
    taps = rs.randn(9)
    for reference in (0, 1):
        for before, tau0, j0 in ((3, 3, 2), (0, 4, 6), (5, 0, 0)):
            k = np.zeros((2, 5, 7))
            k[1, tau0, j0] = 1.0
            got = correlate(x, 0, 0, 120, 0, 120, taps, reference, before, k)
            z = reference_rows(x, 0, 0, 120, -before, 120 - before + 5, taps, reference)
            assert np.array_equal(got[:, 1], z[tau0:tau0 + 120, j0]) and not got[:, 0].any()
            assert not np.signbit(got[:, 0]).any()


def test_t1_is_projects_chain():
    rs = np.random.RandomState(6)
    x = rs.randint(-30000, 30000, size=(200, 13)).astype(np.int16)
    k = rs.randn(6, 1, 13)
    got = correlate(x, 0, 0, 200, 0, 200, [1.0], 0, 0, k)
    with np.errstate(over='ignore'):
        w = k[:, 0, :].T.astype(np.float32)
    assert got.tobytes() == project_chain_f32(x, None, w).tobytes()
