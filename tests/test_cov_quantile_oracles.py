"""The references of tests/test_gpu_cov_quantile_edges.py, on the CPU: the Gram bound with its underflow term against the numpy float64
stand-in on inputs whose products are subnormal, the bound left as it was where they are normal, astype(float64) of 8-byte integers
against Python's int -> float, the order-independence check, and every case of tests/cov_quantile_cases.py driven through the stand-ins
(GramOracleCodec, SelectOracleCodec, StatsOracleCodec) at a smaller shape.  A reference that fails itself here cannot judge the
device."""
import numpy as np
import pytest

from mtscomp_amd import api
from tests import cov_quantile_cases as K
from tests.gram_oracle import (TINY, U, UL, GramOracleCodec, assert_gram_within, assert_order_free, gamma, gram_allowance,
                               gram_bound, reference, tree_height, underflow_term, widen)
from tests.select_oracle import SelectOracleCodec
from tests.stats_oracle import StatsOracleCodec

ROWS, NC, CHUNK = 2 * 1000 + 37, 10, 385                      # (no tiles in the stand-ins: three windows of 999, chunks inside them)


class AllOracleCodec(GramOracleCodec, SelectOracleCodec, StatsOracleCodec):
    """The three stand-ins behind one Reader."""


def _codec():
    return AllOracleCodec(n_lanes=2, capacity_chunks=8)


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


# ---- the bound --------------------------------------------------------------------------------------------------------------------
def test_underflow_term_is_what_the_stand_in_needs(tmp_cfg):
    """float64 BLAS on items whose squares are subnormal: outside the purely relative bound (whose allowance is 0 there), inside the
    bound with n * 2^-1074."""
    x = K.underflow_inexact(ROWS, NC)
    r, dec = K.recording(tmp_cfg, x, CHUNK, _codec())
    worst = K.run_cov(r, dec, teeth=False)
    assert 0 < worst <= 1
    got = r.cov().gram[0]
    ref, ref_err, absgram = reference(dec)
    err = np.abs(got.astype(np.longdouble) - ref)
    h = tree_height(ROWS)
    assert not (err <= gram_bound(h, absgram) + ref_err).all()             # the old form fails the stand-in ...
    assert (err <= gram_bound(h, absgram, ROWS) + ref_err).all()           # ... the new one holds it
    assert float(underflow_term(ROWS)) == ROWS * 2.0 ** -1074 and not underflow_term(0)
    r.close()
    print('stand-in on subnormal products: largest error %.3g units of 2^-1074 in %d rows, error / allowance %.3g'
          % (float(err.max() / TINY), ROWS, worst))


def test_bound_is_the_old_one_where_products_are_normal():
    rs = np.random.RandomState(1)
    for scale in (1.0, 1e-150, 1e150, 3e-154):                               # (3e-154: squares just above the smallest normal)
        x = (1 + rs.rand(500, 4)) * scale
        h = tree_height(500)
        ref, ref_err, absgram = reference(x)
        assert (absgram >= np.finfo(np.float64).tiny).all()
        old = gamma(h + 3) * absgram
        new = gram_bound(h, absgram, 500)
        assert (new >= old).all() and (new - old <= 500 * TINY).all()
        _, allow = gram_allowance(x, h)
        assert (allow - (old + ref_err) <= 500 * TINY).all()
        assert (500 * TINY <= U * absgram)[absgram >= 500 * 2.0 ** -1021].all()
        if scale >= 1.0:
            assert new.tobytes() == old.tobytes()                            # (far from the bottom the term is below the last bit)
        assert_gram_within(x.T @ x, x, h)                                    # and its teeth are what they were
    assert U == 2.0 ** -53 and UL == 2.0 ** -64


def test_widening_of_8_byte_integers_rounds_to_nearest_even():
    """The reference widens with astype(float64); Python's int -> float is correctly rounded, ties to even."""
    i64 = [(1 << 53) + d for d in range(8)] + [-(1 << 53) - d for d in range(8)] + [(1 << 63) - 1, -(1 << 63), -(1 << 63) + 1, (1 << 62) + 512,
                                                                                   -(1 << 62) - 1536, (1 << 62) + 513, 0, -1]
    u64 = [(1 << 53) + d for d in range(8)] + [(1 << 63) - 1, 1 << 63, (1 << 64) - 1, (1 << 64) - 2, (1 << 63) + 1024, (1 << 63) + 3072,
                                               (1 << 63) + 1025, (1 << 64) - 1025, (1 << 64) - 1024]
    for vals, dt in ((i64, np.int64), (u64, np.uint64)):
        a = np.array(vals, dtype=dt)
        assert [int(v) for v in a] == vals
        assert widen(a).tolist() == [float(v) for v in vals]
    assert float((1 << 53) + 1) == 2.0 ** 53 and float((1 << 53) + 3) == 2.0 ** 53 + 4 and float((1 << 64) - 1) == 2.0 ** 64
    assert float((1 << 63) + 1024) == 2.0 ** 63 and float((1 << 63) + 3072) == 2.0 ** 63 + 4096
    for dtype in ('int64', 'uint64'):                                        # and the family's columns hold such values
        x = K.cov_family(dtype, 64, NC)
        ties = [int(v) for v in x[:, 4:9].ravel() if float(int(v)) != int(v)]
        assert len(ties) > 64
        assert widen(x).tolist() == [[float(int(v)) for v in row] for row in x]


def test_order_free_check_sees_what_it_is_for():
    fmax = np.finfo(np.float64).max
    ok = np.array([[fmax, 4.0, 0.0, 1e200], [-fmax, -8.0, 1e-200, -1e200], [fmax, 0.0, np.inf, 3.0]])
    assert_order_free(ok[:2], 0, 2, None)
    assert_order_free(ok, 0, 3, None)                                        # (inf * 0: NaN whatever the order)
    assert_order_free(np.array([[np.inf, 1.0], [np.inf, -1.0]]), 0, 2, None)    # (inf - inf from infinite items: NaN, fused or not)
    for bad in (np.array([[fmax, 1.5], [-fmax, 1.5]]),                      # a product in [max, 2 max): finite when fused
                np.array([[fmax, 0.9], [fmax, 0.9]]),                        # the sum overflows or not with its order
                np.array([[1e154, 1e154]] * 4),
                np.array([[fmax, 8.0], [-fmax, 8.0]])):                      # overflow both ways: NaN unfused, -inf fused
        with pytest.raises(AssertionError, match='order of the sum'):
            assert_order_free(bad, 0, len(bad), None)


# ---- the cases of the GPU file on the stand-ins ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', K.DTYPES)
def test_cov_families(tmp_cfg, dtype):
    r, dec = K.recording(tmp_cfg, K.cov_family(dtype, ROWS, NC), CHUNK, _codec())
    print('%s: largest error / allowance %.3g' % (dtype, K.run_cov(r, dec)))
    r.close()


@pytest.mark.parametrize('e', [-537, -520, -100, 0, 490])
def test_scaled_integers_float64(tmp_cfg, e):
    k = K.small_ints(ROWS, NC)
    r, _ = K.recording(tmp_cfg, np.ldexp(k.astype(np.float64), e), CHUNK, _codec())
    K.run_scaled(r, k, e)
    r.close()


def test_scaled_integers_float32_subnormal_items(tmp_cfg):
    k = K.small_ints(ROWS, NC)
    x = np.ldexp(k.astype(np.float64), -149).astype(np.float32)
    assert (np.abs(x[k != 0]) < np.finfo(np.float32).tiny).all() and np.array_equal(x.astype(np.float64), np.ldexp(k.astype(np.float64), -149))
    r, _ = K.recording(tmp_cfg, x, CHUNK, _codec())
    K.run_scaled(r, k, -149)
    r.close()


@pytest.mark.parametrize('dtype', ['int64', 'uint64'])
def test_scaled_integers_8_byte(tmp_cfg, dtype):
    k = K.small_ints(ROWS, NC, lo=-1023 if dtype == 'int64' else 0, hi=1023)
    r, _ = K.recording(tmp_cfg, (k.astype(np.int64) << 40).astype(dtype), CHUNK, _codec())
    K.run_scaled(r, k, 40)
    r.close()


def test_subnormal_operands_normal_products(tmp_cfg):
    x, k, e = K.mixed_pair(K.small_ints(ROWS, NC))
    r, _ = K.recording(tmp_cfg, x, CHUNK, _codec())
    K.run_mixed(r, x, k, e)
    r.close()


@pytest.mark.parametrize('dtype', K.DTYPES)
def test_quantile_families(tmp_cfg, dtype):
    r, dec = K.recording(tmp_cfg, K.cov_family(dtype, ROWS, NC), CHUNK, _codec())
    K.run_quantile(r, dec, q=(0.0, 0.5, 1.0))
    r.close()


def test_centers_give_zero_keys_ties_and_nan():
    for dtype in ('int8', 'uint64', 'float64'):
        dec = K.cov_family(dtype, 500, 12)
        c = K.centers(dec)
        with np.errstate(invalid='ignore', over='ignore'):
            d = dec.astype(np.float64) - c
        assert (d[:, 0] == 0).any() and (d[:, 4] == 0).any()                 # zero keys
        assert len(np.unique(d[:, 9])) <= (3 if dec.dtype.itemsize == 8 else 1) < len(np.unique(dec[:, 9])) // 10      # massive ties
        assert np.isnan(d[:, 2]).all() and np.isinf(d[:, 6][np.isfinite(dec[:, 6].astype(np.float64))]).all()
    assert (K.cov_family('uint64', 500, 12) >= np.uint64(1 << 63)).sum() > 1000
    z = K.cov_family('float64', 500, 12)[:, 0]
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()   # -0 and +0 about the center 0.0


@pytest.mark.parametrize('dtype', ['uint8', 'int16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64'])
def test_divergence_families(tmp_cfg, dtype):
    x = K.divergence_family(dtype)
    kb = 8 * x.dtype.itemsize
    bits = np.ascontiguousarray(x).view('uint%d' % kb)
    for d in range(kb):                                                      # the family is what its docstring says
        a = np.unique(bits[:, 2 * d])
        if x.dtype.kind != 'f' or len(a) == 2:                               # (a float NaN pattern became 1.0)
            assert len(a) == 2 and int(a[0]) ^ int(a[1]) == 1 << d
    r, dec = K.recording(tmp_cfg, x, 250, _codec())
    print('%s: rounds of a median %d, of a mad %d' % ((dtype,) + K.run_divergence(r, dec, windows=(None, 200))))    # (the stand-in pays per window)
    r.close()


@pytest.mark.parametrize('dtype', K.DTYPES)
def test_identities_between_the_reductions(tmp_cfg, dtype):
    r, dec = K.recording(tmp_cfg, K.cov_family(dtype, ROWS, NC), CHUNK, _codec())
    K.run_consistency(r, dec)
    r.close()
