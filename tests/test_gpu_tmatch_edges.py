"""Reader.correlate and Reader.match_templates on the MI355X at their limits and at every path of their kernels, byte for byte against
tests/correlate_oracle.py and tests/tmatch_oracle.py over the oracle codec's decode, or against literal expectations
(tests/tmatch_cases.py holds the inputs and the checks; tests/test_tmatch_cases.py runs the same cases through the numpy stand-ins
on the CPU and certifies what the inputs reach):
  * k_tmatch_emit in every wave of a block, in 1, 2, 5 and 9 blocks (one bit per row: a block is 65 536 rows), with a ragged last
    thread, sparse, half dense and with every bit set, at every capacity edge, from a second slab that continues from a total past
    2^17, through the Reader's second call after a short first buffer and through the entry point that leaves the events on the device;
  * k_tmatch_best at 64, 65, 1023 and 1024 templates with the maximum at every index, positive and negative, ties in one lane, across
    lanes and with the lower index on the higher lane, non-finite and subnormal rows, and thresholds at the value and the floats either
    side of it, per template -- the scores set by hand through identity templates, which is also correlate at 1024 x 1024;
  * k_tmatch_mask across slab seams where a slab owns 1, R - 1, R, R + 1 and 2 R + 1 rows, on equal peaks at every distance 1 .. R + 1
    on one template and on two, two equal peaks in one row, a plateau and larger peaks R and R + 1 rows later;
  * k_correlate's template chunks of 16 taus at T = 15 .. 255 with one and two column groups, bands and output tiles; 1024 columns,
    1024 templates and 256 taus over two bands and two tiles; every template entry read back by name through impulses; subnormal
    operands whose products are normal."""
import numpy as np
import pytest

from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests import tmatch_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    K.plain_env(monkeypatch)
    for name in ('TMATCH_CALL_BYTES', 'CORRELATE_CALL_BYTES', 'CORRELATE_OUT_BYTES'):      # a whole range is one device call
        monkeypatch.setattr(api, name, 1 << 40)
    return tmp_path


def _make(tmp):
    """One lane on device 0: a call over the whole range is one device call, whatever the number of devices."""
    return lambda x, chunk_rows: K.recording(tmp, x, chunk_rows, codec=api.HipCodec(devices=[0]))


def _dev_entry(tmp, made):
    """mts_dev_match_templates on the file's chunks in device memory; the events stay on the device and are read back."""
    def dev(k, thr, R, cap):
        r = made[0]
        data = (tmp / 'd.cbin').read_bytes()
        cbuf = hip.DevBuffer(len(data) + 256)
        host = np.frombuffer(data + b'\0' * 256, dtype=np.uint8).copy()
        hip._check(hip.lib().mts_dev_copy(0, None, cbuf.at(), hip._ptr(host), host.nbytes, 0), 'mts_dev_copy')
        offs, bounds = np.asarray(r.chunk_offsets, np.int64), np.asarray(r.chunk_bounds, np.int64)
        st, n_ev, res, out = hip.dev_match_templates(cbuf, offs[:-1], np.diff(offs), bounds[:-1], np.diff(bounds), r.n_channels, r.dtype, r._flags(),
                                                     0, r.n_samples, 0, r.n_samples, [1.0], np.arange(r.n_channels), 0, 0, k, thr, R, cap)
        out.free()
        cbuf.free()
        assert st == [hip.CHUNK_OK] * r.n_chunks
        return n_ev, res
    return dev


@pytest.mark.parametrize('rows,chunk,own', K.EMIT_CASES)
def test_emit_in_every_wave_block_and_slab(tmp_cfg, monkeypatch, rows, chunk, own):
    made = []

    def make(x, chunk_rows):
        r, dec = _make(tmp_cfg)(x, chunk_rows)
        made.append(r)
        return r, dec
    out = K.run_emit(make, rows, chunk, own, monkeypatch, dev=_dev_entry(tmp_cfg, made) if rows >= 65537 else None)
    print('emit %d rows: templates -> (sparse, half dense, every row) %r' % (rows, out))
    assert out[1][2] == out[3][2] == rows


@pytest.mark.parametrize('n', K.BEST_NS)
def test_row_maxima_at_every_index_tie_and_threshold(tmp_cfg, n):
    assert K.run_best(_make(tmp_cfg), n) == set(range(n))


@pytest.mark.parametrize('R', [1, 7, 255])
def test_slab_seams_on_plateaus_and_ties(tmp_cfg, monkeypatch, R):
    assert K.run_seams(_make(tmp_cfg), R, monkeypatch) >= 6                # (R = 1: slabs of 1, 2 and 3 rows)


@pytest.mark.parametrize('T', K.EDGE_TS)
def test_template_chunk_and_prefetch_edges(tmp_cfg, T):
    r, dec = _make(tmp_cfg)(K.edge_recording(), K.EDGE_CHUNK)
    K.run_chunk_edges(r, dec, T)
    r.close()


@pytest.mark.parametrize('n_cols,n_out,T', K.LIMIT_SHAPES)
def test_documented_limits(tmp_cfg, n_cols, n_out, T):
    r, dec = _make(tmp_cfg)(synth_int16(0, K.LIMIT_ROWS, 70, 3), 35)
    K.run_limit(r, dec, n_cols, n_out, T)
    r.close()


@pytest.mark.parametrize('before', [0, 128, 256])
def test_longest_templates_over_two_bands_and_tiles(tmp_cfg, before):
    r, dec = _make(tmp_cfg)(synth_int16(0, K.TALL_ROWS, 70, 3), K.TALL_CHUNK)
    K.run_tall(r, dec, before)
    r.close()


def test_impulses_read_every_template_entry_back(tmp_cfg):
    r, _ = _make(tmp_cfg)(K.impulse_recording(), 1000)
    K.run_impulse(r)
    r.close()


@pytest.mark.parametrize('kind', ['x', 'k', 'both'])
def test_subnormal_operands(tmp_cfg, kind):
    want = K.run_subnormal(_make(tmp_cfg), kind)
    assert (want == 0).all() if kind == 'both' else (np.abs(want) >= K.TINY).mean() > 0.5
