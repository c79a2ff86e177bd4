"""The messages of the arguments that detect, waveforms, correlate, match_templates and residual share (taps, reference, the median's
column limit; templates and before for the three template ops): every Reader method against every bad shared argument, the exception
type and its full text held to literals recorded from the commit before the five methods got one parser per argument group.  No device
call is made: every error comes before one."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api
from mtscomp_amd.synth import synth_int16
from tests.residual_oracle import ResidualOracleCodec


class _NoCallCodec(ResidualOracleCodec):
    """Has all five ops for Reader._need_codec; those it adds are never reached."""

    def detect(self, *a, **kw):
        raise AssertionError('a device call')

    waveforms = correlate = detect


K = np.ones((2, 4, 5))                                                   # K = 2 templates of T = 4 rows on the W = 5 channels
INF = K.copy()
INF[1, 2, 3] = np.inf
GOOD = {
    'detect': dict(threshold=1.0, start=10, stop=30),
    'waveforms': dict(sample=[10, 20], before=2, after=2),
    'correlate': dict(templates=K, start=10, stop=30, before=2),
    'match_templates': dict(templates=K, threshold=1.0, start=10, stop=30, before=2),
    'residual': dict(sample=[10, 20], template=[0, 1], amplitude=[1.0, 2.0], templates=K, start=10, stop=30, before=2),
}
TEMPLATE_OPS = ('correlate', 'match_templates', 'residual')
FILTER_CASES = {
    'reference_mean': dict(reference='mean'),
    'taps_empty': dict(taps=[]),
    'taps_8193': dict(taps=np.ones(8193)),
    'taps_nan': dict(taps=[1.0, np.nan]),
    'median_1025_columns': dict(reference='median', channels=[0] * 1025),
}
TEMPLATE_CASES = {
    'templates_1d': dict(templates=np.ones(5)),
    'templates_strings': dict(templates=np.full((2, 4, 5), 'a')),
    'templates_wrong_w': dict(templates=np.ones((2, 4, 4))),
    'templates_t0': dict(templates=np.ones((2, 0, 5))),
    'templates_t257': dict(templates=np.ones((2, 257, 5))),
    'templates_k0': dict(templates=np.ones((0, 4, 5))),
    'templates_k1025': dict(templates=np.ones((1025, 4, 5))),
    'templates_inf': dict(templates=INF),
    'before_minus_1': dict(before=-1),
    'before_t_plus_1': dict(before=5),
    'before_true': dict(before=True),
    'median_1025_columns_templates_to_match': dict(reference='median', channels=[0] * 1025, templates=np.ones((2, 4, 1025))),
}
TABLE = [(op, name, bad) for op in GOOD for name, bad in FILTER_CASES.items()] + \
        [('waveforms', 'median_1025_columns_one_wide', dict(reference='median', channels=[0] * 1025, neighbours=0, channel=[0, 0]))] + \
        [(op, name, bad) for op in TEMPLATE_OPS for name, bad in TEMPLATE_CASES.items()]

_ROWS = "templates have 1 to 256 rows, got %d"
_NUMBERS = "templates must be a (K, T, W) or (T, W) array of numbers"
_TAPS = "taps must be a 1-D sequence of 1 to 8192 finite numbers"
_MEDIAN = "a median reference takes at most 1024 columns, got 1025"
EXPECTED = {
    'reference_mean': "reference must be None or 'median', got 'mean'",
    'taps_empty': _TAPS, 'taps_8193': _TAPS, 'taps_nan': _TAPS,
    ('detect', 'median_1025_columns'): _MEDIAN,
    ('waveforms', 'median_1025_columns'): "a snippet holds at most 1024 positions, got 1025",      # (all columns wide: the width speaks first)
    'median_1025_columns_one_wide': _MEDIAN,
    # (the template ops hold the templates to the channels first, and take no more columns than the median does)
    'median_1025_columns': "templates have 5 columns for 1025 selected channels",
    'median_1025_columns_templates_to_match': "%s takes 1 to 1024 columns, got 1025",
    'templates_1d': _NUMBERS, 'templates_strings': _NUMBERS,
    'templates_wrong_w': "templates have 4 columns for 5 selected channels",
    'templates_t0': _ROWS % 0, 'templates_t257': _ROWS % 257,
    'templates_k0': "%s takes 1 to 1024 templates, got 0", 'templates_k1025': "%s takes 1 to 1024 templates, got 1025",
    'templates_inf': "templates must be finite in float32",
    'before_minus_1': "before must be an int in [0, 4], got -1", 'before_t_plus_1': "before must be an int in [0, 4], got 5",
    'before_true': "before must be an int in [0, 4], got True",
}


@pytest.fixture(scope='module')
def reader(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('messages')
    mp = pytest.MonkeyPatch()
    mp.setattr(api, 'CONFIG_PATH', tmp / '.mtscomp')
    api.set_codec(None)
    codec = _NoCallCodec(n_lanes=1, capacity_chunks=8)
    arr = synth_int16(0, 2000, 5, 9)
    arr.tofile(tmp / 'data.bin')
    mtscomp_amd.compress(tmp / 'data.bin', tmp / 'data.cbin', tmp / 'data.ch', sample_rate=1000., n_channels=5, dtype=arr.dtype, codec=codec,
                         check_after_compress=False)
    r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', codec=codec, check_after_decompress=False)
    yield r, codec
    r.close()
    mp.undo()


def outcome(r, op, bad):
    try:
        getattr(r, op)(**{**GOOD[op], **bad})
    except Exception as e:                                               # noqa: BLE001 (the type is what is compared)
        return type(e).__name__, str(e)
    return None, None


@pytest.mark.parametrize('op,name,bad', TABLE, ids=['%s-%s' % (op, name) for op, name, _ in TABLE])
def test_message_is_the_parents(reader, op, name, bad):
    r, codec = reader
    text = EXPECTED.get((op, name), EXPECTED[name])
    assert outcome(r, op, bad) == ('ValueError', text % op if '%s' in text else text)
    assert not (codec.match_templates_calls or codec.residual_calls or codec.match_residual_calls)
