"""The restatements tests/project_oracle.py holds the GPU results of mts_project to, checked on their own: the vectorised fmaf
against libm's, the float32 chain against the longdouble reference within project_bound (and the bound's teeth), and
api.whitening_weights."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from mtscomp_amd import api
from tests.project_oracle import (TINY, assert_project_within, fmaf_f32, project_bound, project_chain_f32, project_chain_f64,
                                  project_reference)


def _libm_fmaf():
    m = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return m.fmaf


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)])


def _ties():
    """Hand-built double-rounding ties: a * b + c lies a hair above or below the midpoint of two float32, where rounding the
    float64 sum first (to the midpoint) and then to float32 (to even) goes the wrong way."""
    out = []
    for sgn in (1.0, -1.0):
        # c = 1 + ulp/2 is no float32, so build the midpoint from a product: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24: half an ulp of 1
        a = np.float32(1 + 2.0 ** -12)
        for tail in (2.0 ** -60, -2.0 ** -60, 2.0 ** -100, -2.0 ** -100):
            out.append((sgn * a, a, sgn * np.float32(tail)))                       # midpoint +- a hair: must not go to even
        out.append((sgn * a, a, np.float32(0.0)))                                  # the exact midpoint: to even
    return out


def test_fmaf_matches_libm():
    fmaf = _libm_fmaf()
    rs = np.random.RandomState(0)
    n = 50000
    exp = rs.randint(-40, 40, size=(3, n))
    t = (rs.randn(3, n) * 2.0 ** exp).astype(np.float32)
    t[2, ::3] = (-(t[0, ::3].astype(np.float64) * t[1, ::3]) * (1 + rs.randn(len(t[2, ::3])) * 1e-7)).astype(np.float32)    # cancellation
    sub = (rs.randn(3, 2000) * np.array([[1e-20], [1e-20], [1e-40]])).astype(np.float32)                                     # subnormal results
    spec = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38, -3.4e38, 1e-38], np.float32)
    grid = np.array(np.meshgrid(spec, spec, spec, indexing='ij')).reshape(3, -1)
    ties = np.array(_ties(), np.float32).T
    for a, b, c in (t, sub, grid, ties):
        want = np.array([fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
        assert _same(fmaf_f32(a, b, c), want)
    # the ties do tell the exact fmaf from the naive one
    a, b, c = ties
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert not _same(naive, fmaf_f32(a, b, c))


def _families(rs, rows=40, n_cols=13):
    """(name, items, offset, weights): the value families of the GPU tests, small."""
    k = rs.randint(-8, 9, size=(n_cols, 5)).astype(np.float64) / 16
    yield 'small-int/dyadic', rs.randint(-100, 100, size=(rows, n_cols)).astype(np.int16), None, k
    yield 'small-int/dyadic/offset', rs.randint(0, 200, size=(rows, n_cols)).astype(np.uint8), rs.randint(0, 200, size=n_cols) * 1.0, k
    for dt in (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64):
        info = np.iinfo(dt)
        x = rs.randint(info.min // 2, info.max // 2 + 1, size=(rows, n_cols), dtype=np.int64).astype(dt) if dt != np.uint64 else \
            rs.randint(0, 2 ** 63 - 1, size=(rows, n_cols), dtype=np.int64).astype(dt) * 2
        yield 'full-range/%s' % np.dtype(dt).name, x, None, rs.randn(n_cols, 5)
    x16 = rs.randint(32768 - 50, 32768 + 50, size=(rows, n_cols)).astype(np.uint16)
    yield 'mid-scale offset', x16, np.full(n_cols, 32768.0), rs.randn(n_cols, 5)
    for dt in (np.float32, np.float64):
        yield 'randn/%s' % np.dtype(dt).name, (rs.randn(rows, n_cols) * 100).astype(dt), rs.randn(n_cols) * 50, rs.randn(n_cols, 5)
    yield 'subnormal products', (rs.randn(rows, n_cols) * 1e-20).astype(np.float32), None, rs.randn(n_cols, 5) * 1e-20


def test_chain_within_bound_of_the_reference():
    rs = np.random.RandomState(1)
    for name, x, off, w in _families(rs):
        for chain, dt in ((project_chain_f32, np.float32), (project_chain_f64, np.float64)):
            if dt == np.float64 and name == 'subnormal products':
                continue                                               # (subnormal in float32 only)
            assert_project_within(chain(x, off, w), x, off, w, dt), name
        if name.startswith('small-int'):                              # exact: no rounding anywhere
            ref = project_reference(x, off, w)[0]
            assert np.array_equal(project_chain_f32(x, off, w).astype(np.longdouble), ref), name
            assert np.array_equal(project_chain_f64(x, off, w).astype(np.longdouble), ref), name


def test_special_values_propagate():
    x = np.array([[1.0, np.inf, 2.0], [np.nan, 1.0, 1.0], [-0.0, -0.0, -0.0], [1.0, 2.0, 3.0]], np.float32)
    w = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]])
    y = project_chain_f32(x, None, w)
    assert np.isnan(y[0, 0]) and y[0, 1] == np.inf                  # inf * 0 is NaN: zero weights are not skipped
    assert np.isnan(y[1]).all()
    assert np.array_equal(np.signbit(y[2]), [False, False])         # -0 * 1 + (+0) = +0
    assert np.array_equal(y[3], [4.0, 2.0])


def test_bound_has_teeth():
    rs = np.random.RandomState(2)
    for dt_items in (np.int16, np.int32, np.uint16):
        info = np.iinfo(dt_items)
        x = rs.randint(info.min // 2, info.max // 2 + 1, size=(30, 17), dtype=np.int64).astype(dt_items)
        x[x == 0] = 1
        w = rs.choice([-1.0, 1.0], size=(17, 4)) * rs.uniform(0.5, 2.0, size=(17, 4))      # weights of comparable size
        ref, ref_err, absum = project_reference(x, None, w)
        for dt in (np.float32, np.float64):
            allow = project_bound(17, absum, dt) + ref_err
            for j in range(17):                                        # dropping any one column's term leaves the bound
                x2 = x.copy()
                x2[:, j] = 0
                moved = np.abs(project_reference(x2, None, w)[0] - ref).astype(np.float64)
                assert (moved > allow).any(), (dt_items, dt, j)
    assert project_bound(5, 0.0, np.float32) == 8 * TINY[4] and project_bound(8, 0.0, np.float64) == 8 * TINY[8]


def test_whitening_weights():
    rs = np.random.RandomState(3)
    a = rs.randn(12, 40)
    c = a @ a.T / 40 + 0.1 * np.eye(12)
    w = api.whitening_weights(c)
    assert w.dtype == np.float64 and w.shape == (12, 12)
    assert np.array_equal(w, w.T)
    assert np.abs(w @ c @ w.T - np.eye(12)).max() <= 1e-9
    w2 = api.whitening_weights(c, eps=0.5)
    lam, e = np.linalg.eigh(c)
    assert np.allclose(w2, (e / np.sqrt(lam + 0.5)) @ e.T, rtol=0, atol=1e-12)
    sing = np.ones((3, 3))
    with pytest.raises(ValueError):
        api.whitening_weights(sing)
    assert np.isfinite(api.whitening_weights(sing, eps=1e-3)).all()
    for bad in (np.ones((3, 4)), np.ones(3), np.zeros((0, 0)), np.array([[1.0, np.nan], [np.nan, 1.0]]), np.array([[np.inf, 0], [0, 1.0]])):
        with pytest.raises(ValueError):
            api.whitening_weights(bad)
    for bad_eps in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            api.whitening_weights(c, eps=bad_eps)
