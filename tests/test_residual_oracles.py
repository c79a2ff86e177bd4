"""The two restatements of the residual's definition in tests/residual_oracle.py -- event after event on whole template rows, and one
scalar chain per entry -- held equal byte for byte on random and adversarial event lists, and the properties that follow from the
definition: order, stitching, the empty list, the scores of the residual."""
import numpy as np

from mtscomp_amd import api
from tests.correlate_oracle import FILL, correlate, correlate_chain, reference_rows
from tests.residual_oracle import (match_residual, residual, residual_brute, residual_scores, sort_events, subtract_rows, subtract_rows_brute,
                                   subtract_rows_t1)
from tests.tmatch_oracle import match_templates

TAPS9 = np.random.RandomState(1).randn(9)


def _canon(z):
    z = np.array(z, np.float32)
    z[np.isnan(z)] = FILL
    return z.tobytes()


def _events(rs, n, rows, K, lo=None, hi=None):
    return (rs.randint(0 if lo is None else lo, rows if hi is None else hi, n), rs.randint(0, K, n), (rs.randn(n) * 2).astype(np.float32))


def test_random_lists_agree():
    rs = np.random.RandomState(0)
    for rows, nc, K, T, before, n, taps, ref, dtype in ((60, 3, 2, 5, 2, 12, [1.0], 0, np.int16), (50, 5, 3, 7, 0, 30, TAPS9, 1, np.int16),
                                                        (40, 4, 1, 1, 1, 25, [1.0], 1, np.float32), (45, 2, 2, 16, 16, 10, TAPS9, 0, np.float32)):
        x = (rs.randn(rows, nc) * 50).astype(dtype)
        k = rs.randn(K, T, nc)
        ev = _events(rs, n, rows, K)
        for i0, i1 in ((0, rows), (7, 31), (rows - 1, rows)):
            a = residual(x, 0, 0, rows, i0, i1, taps, ref, before, k, *ev)
            assert a.dtype == np.float32 and a.shape == (i1 - i0, nc)
            assert a.tobytes() == residual_brute(x, 0, 0, rows, i0, i1, taps, ref, before, k, *ev).tobytes()
        whole = residual(x, 0, 0, rows, 0, rows, taps, ref, before, k, *ev)
        assert whole.tobytes() != reference_rows(x, 0, 0, rows, 0, rows, taps, ref).tobytes()         # (something was subtracted)
        # stitching, and rows given with a halo (x_row0 > 0, as a call's chunks give them)
        assert whole[10:33].tobytes() == residual(x, 0, 0, rows, 10, 33, taps, ref, before, k, *ev).tobytes()
        if len(taps) == 1:
            assert whole[10:33].tobytes() == residual(x[10:33], 10, 0, rows, 10, 33, taps, ref, before, k, *ev).tobytes()
        # events that cover none of the rows asked for change nothing
        s = sort_events(*ev)
        near = (s[0] - before < 33) & (s[0] - before + T > 10)
        assert whole[10:33].tobytes() == residual(x, 0, 0, rows, 10, 33, taps, ref, before, k, *(v[near] for v in s)).tobytes()
        # an empty list is z
        none = residual(x, 0, 0, rows, 0, rows, taps, ref, before, k, [], [], [])
        assert none.tobytes() == _canon(reference_rows(x, 0, 0, rows, 0, rows, taps, ref))


def test_adversarial_lists_agree():
    rs = np.random.RandomState(3)
    rows, nc, K, T, before = 40, 3, 3, 6, 2
    k = rs.randn(K, T, nc)
    k[1, 2] = 0.0                                                       # zero template entries are not skipped
    z0 = (rs.randn(rows, nc) * 5).astype(np.float32)
    z0[rs.rand(rows, nc) < 0.3] = -0.0                                  # z entries of -0
    z0[12, 1] = np.inf
    lists = {
        'ties': ([10, 10, 10, 4, 4], [0, 1, 2, 2, 0], [1.0, -2.0, 0.5, 3.0, 3.0]),
        'deep': ([20, 21, 19, 20, 22, 20], [0, 1, 2, 1, 0, 2], [1.5, 0.25, -1.0, 2.0, 1.0, -0.75]),             # >= 4 events on rows 20 .. 23
        'ends': ([0, 0, 1, rows - 1, rows - 1, rows - 2], [0, 1, 2, 0, 1, 2], [1.0, 2.0, 3.0, -1.0, 0.5, 2.5]),  # windows over both ends
        'zero': ([8, 9, 30], [0, 1, 2], [0.0, -0.0, 0.0]),                                                     # amplitude +-0
        'huge': ([15, 15, 16, 17], [0, 0, 1, 2], [3e38, -3e38, 3e38, 3e38]),                                    # +-inf, then NaN
    }
    for name, ev in lists.items():
        a = subtract_rows(z0.copy(), 0, 0, rows, *ev, before, k)
        b = subtract_rows_brute(z0, 0, 0, rows, *ev, before, k)
        assert _canon(a) == _canon(b), name
        # a window of rows, with the rows outside the recording left alone
        z = np.concatenate([np.zeros((4, nc), np.float32), z0[:10]])
        a = subtract_rows(z.copy(), -4, 0, rows, *ev, before, k)
        assert _canon(a) == _canon(subtract_rows_brute(z, -4, 0, rows, *ev, before, k)), name
        assert a[:4].tobytes() == z[:4].tobytes()
    huge = subtract_rows(z0.copy(), 0, 0, rows, *lists['huge'], before, k)
    # (the product inside an fmaf is not rounded: the residual overflows to +-inf and stays there; its scores are where inf - inf and
    # inf * 0 give a NaN)
    assert np.isposinf(huge).any() and np.isneginf(huge).any() and np.isnan(correlate_chain(huge, k)).any()
    # amplitude 0 with -0 in z: a row that no event covers keeps its -0, and so does a covered -0 under a product of -0
    zero = subtract_rows(z0.copy(), 0, 0, rows, *lists['zero'], before, k)
    assert zero[:6].tobytes() == z0[:6].tobytes() and np.signbit(zero[:6]).any()
    kp = np.abs(k)
    zz = np.full((rows, nc), -0.0, np.float32)
    assert np.signbit(subtract_rows(zz.copy(), 0, 0, rows, [8], [0], [0.0], before, kp)).all()      # fmaf(-0, K, -0) = -0: a masked step would not be
    assert not np.signbit(subtract_rows(zz.copy(), 0, 0, rows, [8], [0], [-0.0], before, kp)[6:12]).any()   # fmaf(+0, K, -0) = +0 under the window ...
    assert np.signbit(subtract_rows(zz.copy(), 0, 0, rows, [8], [0], [-0.0], before, kp)[:6]).all()         # ... and nowhere else
    # ties keep list order: swapping two events of one sample changes the bytes when the chain does not commute
    x = np.full((rows, nc), 1, np.float32)
    kk = np.ones((2, 1, nc), np.float32)
    one = subtract_rows(x.copy(), 0, 0, rows, [5, 5], [0, 1], [1e8, 5.0], 0, kk)       # 1 - 1e8 -> -1e8 (spacing 8), - 5 -> -100000008
    two = subtract_rows(x.copy(), 0, 0, rows, [5, 5], [1, 0], [5.0, 1e8], 0, kk)       # 1 - 5 = -4, - 1e8 -> -100000004 -> to even: -1e8
    assert one[5].tolist() == [-100000008.0] * nc and two[5].tolist() == [-100000000.0] * nc
    assert one[4].tolist() == [1.0] * nc and one[6].tolist() == [1.0] * nc


def test_one_row_templates_by_rank():
    rs = np.random.RandomState(8)
    z0 = (rs.randn(300, 4) * 5).astype(np.float32)
    k = rs.randn(3, 1, 4)
    ev = (rs.randint(0, 300, 2000), rs.randint(0, 3, 2000), (rs.randn(2000) * 2).astype(np.float32))          # ~7 deep on every row
    for before, (r0, vb, ve) in ((0, (0, 0, 300)), (1, (0, 0, 300)), (0, (-5, 0, 290))):
        assert subtract_rows_t1(z0.copy(), r0, vb, ve, *ev, before, k).tobytes() == subtract_rows(z0.copy(), r0, vb, ve, *ev, before, k).tobytes()
    assert subtract_rows_t1(z0.copy(), 0, 0, 300, [], [], [], 0, k).tobytes() == z0.tobytes()


def test_scores_of_the_residual():
    rs = np.random.RandomState(5)
    rows, nc, K, T, before = 80, 4, 2, 5, 2
    x = (rs.randn(rows, nc) * 30).astype(np.int16)
    k = rs.randn(K, T, nc)
    ev = _events(rs, 9, rows, K)
    for taps, ref in (([1.0], 0), (TAPS9, 1)):
        sc = residual_scores(x, 0, 0, rows, 0, rows, taps, ref, before, k, *ev)
        # the chain on z' inside the recording and +0 outside it
        zp = residual(x, 0, 0, rows, 0, rows, taps, ref, before, k, *ev)
        pad = np.concatenate([np.zeros((before, nc), np.float32), zp, np.zeros((T - before - 1, nc), np.float32)])
        assert sc.tobytes() == correlate_chain(pad, k).tobytes()
        assert sc[20:50].tobytes() == residual_scores(x, 0, 0, rows, 20, 50, taps, ref, before, k, *ev).tobytes()
        # an empty list: correlate and match_templates themselves
        assert residual_scores(x, 0, 0, rows, 0, rows, taps, ref, before, k, [], [], []).tobytes() == correlate(x, 0, 0, rows, 0, rows, taps, ref, before, k).tobytes()
        thr = np.percentile(sc, 80, axis=0).astype(np.float32)
        got = match_residual(x, 0, 0, rows, 3, 70, taps, ref, before, k, thr, 3, [], [], [])
        assert got[0].size and all(a.tobytes() == b.tobytes() for a, b in zip(got, match_templates(x, 0, 0, rows, 3, 70, taps, ref, before, k, thr, 3)))
        whole = match_residual(x, 0, 0, rows, 0, rows, taps, ref, before, k, thr, 3, *ev)
        parts = [match_residual(x, 0, 0, rows, a, b, taps, ref, before, k, thr, 3, *ev) for a, b in ((0, 37), (37, rows))]
        assert whole[0].size and all(np.concatenate([p[i] for p in parts]).tobytes() == whole[i].tobytes() for i in range(3))


def test_template_amplitudes():
    rs = np.random.RandomState(2)
    k = rs.randn(4, 6, 5) * 3
    score = (rs.randn(50) * 100).astype(np.float32)
    tpl = rs.randint(0, 4, 50)
    amp = api.template_amplitudes(score, tpl, k)
    norm = [float(np.sum(k[i].astype(np.float32).astype(np.float64) ** 2)) for i in range(4)]
    assert amp.dtype == np.float32 and amp.tolist() == [np.float32(float(s) / norm[t]) for s, t in zip(score, tpl)]
    assert api.template_amplitudes(score[:3], [0, 0, 0], k[0]).tolist() == [np.float32(float(s) / norm[0]) for s in score[:3]]
    assert api.template_amplitudes([], [], k).shape == (0,)
