"""Reader.detect on the MI355X at the widths, slab sizes and event densities of the real workload, byte for byte against
tests/detect_oracle.py over the oracle codec's decode (tests/detect_cases.py holds the inputs and the checks; tests/test_detect_oracles.py
runs the same cases through the numpy stand-in on the CPU):
  * k_row_median at every network size P = 2 .. 1024: n = P - 1 (one padding key), P (none) and P + 1 (nearly half padding), in order
    and shuffled with repeats, on random, tied, sorted, constant, NaN, infinite, overflowing and subnormal rows, read back whole
    through a dump of z (threshold 2^-126, or 2^-149 for the subnormal rows; no neighbours);
  * k_detect_scan with 256, 257 and 513 blocks in one slab (1, 2 and 3 blocks per thread, the last thread ragged), three words per row
    at large block indices, and a second slab that continues from a large total; sparse and dense, every capacity edge;
  * k_detect_count / k_detect_emit with every bit of every word set, and the Reader's second call after a short first buffer;
  * slab seams where a slab owns 1, R - 1, R, R + 1 and 2 R + 1 rows, on ties at every distance 1 .. R + 1, a plateau and larger peaks
    R and R + 1 rows later, with the median reference subtracted in the halo rows two slabs share;
  * ties across the 64-position words at spread 1, 31 and 32, and the clips at positions 0 and n - 1;
  * v > threshold at the float32 threshold itself and the floats either side, per column."""
import numpy as np
import pytest

from mtscomp_amd import api
from tests import detect_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    K.plain_env(monkeypatch)
    return tmp_path


def _make(tmp):
    """One lane on device 0: a call over the whole range is one device call, whatever the number of devices."""
    return lambda x, chunk_rows: K.recording(tmp, x, chunk_rows, codec=api.HipCodec(devices=[0]))


@pytest.mark.parametrize('dtype', ['float32', 'int16'])
def test_median_every_network_size(tmp_cfg, monkeypatch, dtype):
    """P = 2, 2, 4, 64, 64, 128, 128, 128, 256, 256, 256, 512, 512, 512, 1024, 1024, 1024 for the n of K.MEDIAN_NS."""
    assert sorted({K.network_size(n) for n in K.MEDIAN_NS}) == [2, 4, 64, 128, 256, 512, 1024]
    r, dec = _make(tmp_cfg)(K.median_recording(dtype), 64)
    seen = K.run_median(r, dec)
    print('median %s: n -> (share of the random rows, dump events, ordinary events, subnormal amplitudes) %r' % (dtype, seen))
    spy = K.Spy(monkeypatch, r)
    with pytest.raises(ValueError, match='at most 1024'):
        r.detect(1.0, channels=list(range(1024)) + [5], reference='median')
    assert not spy.calls                                              # ... and nothing reached the device
    r.detect(1e30, channels=list(range(1024)) + [5])                 # (without a reference 1025 columns are fine)
    assert len(spy.calls) == 1
    r.close()


# (rows, columns, chunk rows, blocks of the slab, blocks per scan thread, rows a slab owns or None: one slab)
SCAN_CASES = [(262144, 1, 40000, 256, 1, None),                      # the last shape on the one-block-per-thread path
              (262145, 1, 40000, 257, 2, None),                      # the first with two; threads 129 .. 255 own nothing
              (2 * 262144 + 7, 1, 50000, 513, 3, None),              # three, the last thread ragged
              (87400, 129, 20000, 257, 2, None),                     # three words per row
              (2 * 262144 + 7, 1, 50000, 257, 2, 262150)]            # two slabs of 257 blocks: the second scan starts from a large total


@pytest.mark.parametrize('rows,nc,chunk,blocks,per,own', SCAN_CASES)
def test_scan_beyond_256_blocks(tmp_cfg, monkeypatch, rows, nc, chunk, blocks, per, own):
    for slab in ([rows] if own is None else [own, rows - own]):
        words, b, p = K.scan_shape(slab, nc)
        assert (b, p) == (blocks, per) and (words > 262144) == (per > 1)
    x = K.spiky_int8(rows, nc, 4000, rows % 1000 + nc)
    r, dec = _make(tmp_cfg)(x, chunk)
    n_sparse, total = K.run_scan(r, dec, monkeypatch, caps=K.SCAN_CAPS, slab_own=own)
    assert 2000 <= n_sparse <= 4000 and total >= 0.99 * rows * nc
    r.close()


@pytest.mark.parametrize('kind', [0, 1])
def test_dense_events_and_second_call(tmp_cfg, monkeypatch, kind):
    mask = K.dense_masks(3000, 70)[kind]
    r, _ = _make(tmp_cfg)(np.where(mask, 7, 0).astype(np.int16), 700)
    K.run_dense(r, mask, monkeypatch, r.n_chunks)
    r.close()


@pytest.mark.parametrize('R', [1, 7, 255])
def test_slab_seams_on_plateaus_and_ties(tmp_cfg, monkeypatch, R):
    assert K.run_seams(_make(tmp_cfg), R, monkeypatch) >= 12             # (R = 1: slabs of 1, 2 and 3 rows)


def test_word_seams_and_spread(tmp_cfg):
    x, marks = K.word_recording()
    r, dec = _make(tmp_cfg)(x, 100)
    K.run_words(r, dec, marks)
    r.close()


def test_threshold_is_strict_and_per_column(tmp_cfg):
    x, vals = K.threshold_recording()
    r, dec = _make(tmp_cfg)(x, 16)
    K.run_threshold(r, dec, vals)
    r.close()
