"""mts_last_error() of the C entries of detect, waveforms, correlate, match_templates and residual for one bad shared argument each,
as (the keywords of the calling test's `call`, the full text).  The texts were recorded from the library of the commit before the
five runs got one check of the filter arguments and one of the templates; `op` is the name the entry's messages begin with.  The
calls they belong to: 100 rows x 4 channels in one chunk, valid rows [0, 100), rows [10, 90), two taps, columns (0, 1); the template
ops with 2 templates of 3 rows, before = 1."""
import numpy as np

_NAN = np.ones((2, 3, 2), np.float32)
_NAN[1, 2, 1] = np.nan
_INF = np.ones((2, 3, 2), np.float32)
_INF[0, 0, 0] = np.inf


def filter_errors(op, rows_too=True):
    """taps, reference and the valid rows.  rows_too: the op takes rows [rb, re) within [vb, ve), so valid rows that do not hold them are
    'rows invalid' as well."""
    rows = [dict(vb=50, ve=20), dict(vb=-1)] + ([dict(vb=20), dict(ve=80)] if rows_too else [])
    return [(dict(ref=2), '%s: reference 2 (0 none, 1 median)' % op), (dict(ref=-1), '%s: reference -1 (0 none, 1 median)' % op),
            (dict(taps=()), '%s: 0 taps (1 .. 8192)' % op), (dict(taps=np.ones(8193)), '%s: 8193 taps (1 .. 8192)' % op),
            (dict(taps=(np.nan,)), '%s: tap 0 is not finite' % op), (dict(taps=(1.0, np.inf)), '%s: tap 1 is not finite' % op)] + \
           [(bad, '%s: rows invalid' % op) for bad in rows]


def wide_errors(op):
    """The columns of detect and waveforms: any number a grid holds, at most 1024 under a median."""
    return [(dict(cols=()), '%s: n_channels, n_chunks or columns invalid' % op),
            (dict(ref=1, cols=[0] * 1025), '%s: a median reference over 1025 columns (<= 1024)' % op)]


def template_errors(op):
    """The columns and the templates of correlate, match_templates and residual."""
    return [(dict(cols=()), '%s: 0 columns (1 .. 1024)' % op), (dict(cols=[0] * 1025), '%s: 1025 columns (1 .. 1024)' % op),
            (dict(ref=1, cols=[0] * 1025), '%s: 1025 columns (1 .. 1024)' % op),
            (dict(T=0), '%s: templates of 0 rows (1 .. 256)' % op), (dict(T=257), '%s: templates of 257 rows (1 .. 256)' % op),
            (dict(T=-1), '%s: templates of -1 rows (1 .. 256)' % op),
            (dict(before=-1), '%s: before -1 (0 .. 3)' % op), (dict(before=4), '%s: before 4 (0 .. 3)' % op),
            (dict(K=0), '%s: 0 templates (1 .. 1024)' % op), (dict(K=1025), '%s: 1025 templates (1 .. 1024)' % op),
            (dict(K=-2), '%s: -2 templates (1 .. 1024)' % op), (dict(templates=False), '%s: 2 templates (1 .. 1024)' % op),
            (dict(tpl=_NAN), '%s: template entry (1, 2, 1) is not finite' % op), (dict(tpl=_INF), '%s: template entry (0, 0, 0) is not finite' % op)]
