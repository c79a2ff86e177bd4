"""Reader.cov (k_gram, k_gram_colsum) and Reader.quantile / median / mad (k_rank_hist) on the MI355X on every item type, value family
and key mode, against references that share none of the kernels' arithmetic (tests/cov_quantile_cases.py holds the inputs and the
checks; tests/test_cov_quantile_oracles.py runs the same cases through the numpy stand-ins on the CPU):
  * cov: all ten item types (every k_gram / k_gram_colsum instantiation) on full-range, constant min / max, alternating and special
    float columns -- exact types and integer sums bit for bit against numpy int64, the others within gram_bound --, the widening of
    8-byte integers at its ties, and float64 magnitudes whose products overflow, chosen so that the reference owns the outcome;
  * float items k * 2^e whose Gram is exact in any order, compared by bytes down to e = -537 (every product an exact subnormal),
    float32 subnormal items, subnormal operands with normal products, and 8-byte integers k * 2^40: a flush anywhere in the kernel
    changes bytes here;
  * products that underflow inexactly, against the bound's n * 2^-1074;
  * quantile / median / mad: all ten types in the three key modes (every k_rank_hist instantiation) on the same families, with
    centers that give zero keys, massive ties and NaN / +-inf keys; and columns whose median candidates first differ at every bit
    of every key width, so that the lanes of one wave carry different (prefix, shift) states down to the lowest digit;
  * cov().sum == window_stats().sum, quantile(0 / 1) == window_stats().min / max, diag(gram) == window_stats().sumsq.
One recording shape serves nearly all of it: 2 * 4096 + 37 rows x 70 columns in chunks of 1537 rows, windows None, 4096, 4097, 999,
a range from row 3, and window=1 over 64 rows."""
import numpy as np
import pytest

from mtscomp_amd import api
from tests import cov_quantile_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


# ---- cov ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', K.DTYPES)
def test_cov_every_item_type(tmp_cfg, dtype):
    r, dec = K.recording(tmp_cfg, K.cov_family(dtype), K.CHUNK)
    print('cov %s: largest error / allowance %.3g' % (dtype, K.run_cov(r, dec)))
    r.close()


@pytest.mark.parametrize('e', [-537, -520, -100, 0, 490])
def test_cov_scaled_integers_float64_by_bytes(tmp_cfg, e):
    """e = -537: every product is an exact subnormal; -520: the products are subnormal and their sums cross into the normal range."""
    k = K.small_ints()
    r, _ = K.recording(tmp_cfg, np.ldexp(k.astype(np.float64), e), K.CHUNK)
    K.run_scaled(r, k, e)
    r.close()


def test_cov_float32_subnormal_items_by_bytes(tmp_cfg):
    k = K.small_ints()
    r, _ = K.recording(tmp_cfg, np.ldexp(k.astype(np.float64), -149).astype(np.float32), K.CHUNK)
    K.run_scaled(r, k, -149)
    r.close()


def test_cov_subnormal_operands_normal_products_by_bytes(tmp_cfg):
    x, k, e = K.mixed_pair(K.small_ints())
    r, _ = K.recording(tmp_cfg, x, K.CHUNK)
    K.run_mixed(r, x, k, e)
    r.close()


@pytest.mark.parametrize('dtype', ['int64', 'uint64'])
def test_cov_8_byte_integers_exact_case_by_bytes(tmp_cfg, dtype):
    k = K.small_ints(lo=-1023 if dtype == 'int64' else 0, hi=1023)
    r, _ = K.recording(tmp_cfg, (k.astype(np.int64) << 40).astype(dtype), K.CHUNK)
    K.run_scaled(r, k, 40)
    r.close()


def test_cov_products_that_underflow_inexactly(tmp_cfg):
    """(1 + rand) * 2e-162 and randn * 1e-310: the squares round in the subnormal range; the relative part of the bound is 0 there.
    No teeth at these magnitudes (dropping a row moves less than n * 2^-1074): the exact cases above supply them."""
    r, dec = K.recording(tmp_cfg, K.underflow_inexact(), K.CHUNK)
    print('cov underflow: largest error / allowance %.3g' % K.run_cov(r, dec, teeth=False))
    r.close()


# ---- quantile / median / mad ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', K.DTYPES)
def test_quantile_every_item_type_and_key_mode(tmp_cfg, dtype):
    r, dec = K.recording(tmp_cfg, K.cov_family(dtype), K.CHUNK)
    K.run_quantile(r, dec)
    r.close()


@pytest.mark.parametrize('dtype', ['uint8', 'int16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64'])
def test_quantile_candidates_that_diverge_at_every_bit(tmp_cfg, dtype):
    r, dec = K.recording(tmp_cfg, K.divergence_family(dtype), 250)
    print('%s: %d columns, rounds of a median %d, of a mad %d' % ((dtype, dec.shape[1]) + K.run_divergence(r, dec)))
    r.close()


# ---- identities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', K.DTYPES)
def test_identities_between_the_reductions(tmp_cfg, dtype):
    r, dec = K.recording(tmp_cfg, K.cov_family(dtype), K.CHUNK)
    K.run_consistency(r, dec)
    r.close()
