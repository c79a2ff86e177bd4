"""Test-only restatements of mts_waveform_features in numpy: the definition of include/mtscomp_hip.h twice -- vectorised (the snippets
of tests/waveforms_oracle.py, one exact fmaf over whole arrays per tau) and by brute force (a scalar chain per (e, p, w) with libm's
fmaf) -- and a lane codec built on the first so that the CPU suite drives Reader.waveform_features (argument handling, order, calls,
lanes, cache use, errors) and can check bit-identity."""
import numpy as np

from tests.correlate_oracle import _libm_fmaf
from tests.project_oracle import fmaf_f32
from tests.waveforms_oracle import FILL, WaveformsOracleCodec, waveforms

MAX_COMPONENTS, MAX_BASIS = 32, 8192


def basis32(basis):
    """The basis as the call takes it: float32 (P, T), every entry finite."""
    b = np.ascontiguousarray(np.asarray(basis, dtype=np.float32))
    assert b.ndim == 2 and np.isfinite(b).all()
    return b


def chain(wave, basis):
    """features (n, P, W) of snippets wave (n, T, W): acc = +0; acc = fmaf(wave[:, tau], basis[p, tau], acc) for tau = 0 .. T - 1; every
    NaN stored with the bits of FILL."""
    wave, b = np.asarray(wave, dtype=np.float32), basis32(basis)
    n, T, W = wave.shape
    assert b.shape[1] == T
    acc = np.zeros((n, b.shape[0], W), np.float32)
    for tau in range(T):
        acc = fmaf_f32(wave[:, tau, None, :], b[None, :, tau, None], acc)
    acc[np.isnan(acc)] = FILL
    return acc


def features(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width, basis):
    """features float32 (n, P, width).  x: the selected columns of file rows [x_row0, x_row0 + len(x)), any item type; [vb, ve): the
    recording; reference 0 / 1; ev_row any order."""
    return chain(waveforms(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width)[0], basis)


# ---- the same definition by brute force: one scalar chain per (e, p, w), libm's fmaf ----------------------------------------------
def chain_brute(wave, basis):
    fmaf = _libm_fmaf()
    wave, b = np.asarray(wave, dtype=np.float32), basis32(basis)
    n, T, W = wave.shape
    out = np.empty((n, b.shape[0], W), np.float32)
    for e in range(n):
        for p in range(b.shape[0]):
            for w in range(W):
                acc = np.float32(0.0)
                for tau in range(T):
                    acc = fmaf(wave[e, tau, w], b[p, tau], acc)
                out[e, p, w] = FILL if np.isnan(acc) else acc
    return out


def features_brute(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width, basis):
    from tests.waveforms_oracle import waveforms_brute
    return chain_brute(waveforms_brute(x, x_row0, vb, ve, taps, reference, ev_row, ev_col0, before, after, width)[0], basis)


class FeaturesOracleCodec(WaveformsOracleCodec):
    """WaveformsOracleCodec + waveform_features restated in numpy, chunks read as waveforms reads them.  Records (lane, keys, lens,
    n_events) of every waveform_features call."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.waveform_features_calls = []
        self.miss_next_waveform_features = False     # simulate an entry dropped between the query and the call

    def waveform_features(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols,
                          reference, ev_row, ev_col0, before, after, width, basis, lane=None):
        ev_row, ev_col0 = np.asarray(ev_row, dtype=np.int64), np.asarray(ev_col0, dtype=np.int64)
        self.waveform_features_calls.append((lane, [int(k) for k in keys], [int(n) for n in lens], int(ev_row.size)))
        cols = np.asarray(cols, dtype=np.int64)
        taps = np.asarray(taps, dtype=np.float64)
        assert cols.size and (cols >= 0).all() and (cols < n_channels).all() and reference in (0, 1)
        assert before >= 0 and after >= 0 and 1 <= before + after <= 4096 and 1 <= width <= 1024
        assert isinstance(basis, np.ndarray) and basis.dtype == np.float32 and basis.ndim == 2 and basis.shape[1] == before + after, 'basis'
        assert 1 <= basis.shape[0] <= MAX_COMPONENTS and basis.size <= MAX_BASIS and np.isfinite(basis).all(), 'basis'
        assert ev_row.size and (np.diff(ev_row) >= 0).all() and valid_begin <= ev_row[0] and ev_row[-1] < valid_end, 'events'
        assert all(int(row0[i]) == int(row0[i - 1]) + int(n_rows[i - 1]) for i in range(1, len(keys))), 'chunks not adjacent'
        half = (taps.size - 1) // 2
        lo, hi = max(valid_begin, int(ev_row[0]) - before + half - (taps.size - 1)), min(valid_end, int(ev_row[-1]) + after + half)
        assert int(row0[0]) <= lo and hi <= int(row0[-1]) + int(n_rows[-1]), 'the chunks do not cover the rows read'
        status, arrays = self._call_chunks('waveform_features', cache_id, keys, cdata, offs, lens, n_rows, n_channels, np.dtype(dtype), flags,
                                           fill=True)
        x = np.concatenate(arrays, axis=0)[:, cols]
        return status, features(x, int(row0[0]), valid_begin, valid_end, taps, reference, ev_row, ev_col0, before, after, width, basis)
