"""Host side of the drop-in: mtscomp's ``compress()/decompress()/Writer/Reader`` API and ``.cbin/.ch``
on-disk format, with the per-chunk codec running on MI355X through ``libmtscomp_hip.so``.

The interface mirrors /root/reference/mtscomp.py (names, argument meaning, error behaviour); every
public item cites the reference lines it stands in for.  What changed is below the interface:

* ``Writer.compress_batch`` hands a whole batch of chunks to ``mts_compress_chunks`` (one C-ABI call
  per device) instead of ``pool.map(self._compress_chunk, ...)`` (mtscomp.py:399-423);
* ``Reader.decompress_chunks`` / ``__getitem__`` hand all missing chunks to ``mts_decompress_chunks``
  instead of ``pool.map(self._decompress_chunk, ...)`` (mtscomp.py:645-650, 810-812);
* chunks are sharded round-robin over the visible GPUs (chunk i -> device i mod G); the only
  cross-device step is the host-side gather of compressed sizes into ``chunk_offsets``.

There is no CPU implementation of the codec in this package: the codec object is ``HipCodec`` and it
raises if the HIP library or a gfx950 device is missing.
"""
import bisect
import hashlib
import json
import logging
import multiprocessing as mp
import os
import threading
import os.path as op
from collections import OrderedDict
from fractions import Fraction
from multiprocessing.dummy import Pool as ThreadPool
from pathlib import Path
from threading import Lock

import numpy as np

from . import hip

__version__ = '0.1.0'
FORMAT_VERSION = '1.0'          # mtscomp.py:41

__all__ = ('load_raw_data', 'Writer', 'Reader', 'compress', 'decompress', 'check', 'diff_along_axis',
           'cumsum_along_axis', 'read_config', 'write_config', 'add_default_handler', 'HipCodec')

# mtscomp.py:46-57 -- same keys, same defaults; the .ch header only ever sees the reference's keys.
DEFAULT_CONFIG = tuple(dict(
    algorithm='zlib',
    cache_size=10,
    check_after_compress=True,
    check_after_decompress=True,
    chunk_duration=1.,
    chunk_order='F',
    comp_level=-1,              # stored in the header, never passed to the codec (mtscomp.py:394)
    do_spatial_diff=False,
    do_time_diff=True,
    n_threads=mp.cpu_count(),   # kept for compatibility; the device path does not use host threads
).items())

CHECK_ATOL = 1e-16              # mtscomp.py:59
CRITICAL_ERROR_URL = "https://github.com/int-brain-lab/mtscomp/issues/new?title=Critical+error"
DEFAULT_BATCH_CHUNKS = 64       # chunks handed to one device call
TOFILE_PIECE_CHUNKS = 8         # chunks per piece of Reader.tofile (decode of one piece under the file writes of the one before)
TOFILE_WRITERS = 4              # threads writing a piece: a fresh tmpfs file takes ~6.5 GB/s whatever their number (its pages are allocated and zeroed under the inode's lock), an existing file written over in place 6-9 GB/s from four (round 5: 2 against 4 writers, new files 2.8-6.2 / 4.0-5.1 GB/s from call to call, over existing files 6.3-8.9 / 6.7-9.0)
DEFAULT_DEVICE_CACHE_GB = 32    # decoded chunks a Reader may keep in HBM for slicing (allocated as touched; env MTSCOMP_DEVICE_CACHE_GB, 0 = off)
DEVICE_CACHE_MAX_CHUNKS = 8     # longer slices are streamed through the host path instead of the cache
READ_AHEAD_MAX = int(os.environ.get('MTSCOMP_READ_AHEAD', 4))   # chunks a cold slice may decode ahead of itself into the device cache (0 = off)
MAP_CDATA = os.environ.get('MTSCOMP_MAP_CDATA', '1') not in ('', '0')      # slices read their compressed bytes out of a mapping of the .cbin (0: preadv into page-locked memory)
PREAD_THREADS = int(os.environ.get('MTSCOMP_PREAD_THREADS', 8))      # threads that read the compressed bytes of a slice's missing chunks (a few MB and more)
WINDOW_STATS_CALL_BYTES = 1 << 30      # Reader.window_stats: compressed bytes per device call (a longer range is split on chunk boundaries)
WINDOW_STATS_SLAB_BYTES = 1 << 30      # ... and partial results per call on the device (one per column and tile of <= 512 rows of a window)
DETECT_CALL_BYTES = 1 << 30            # Reader.detect: compressed bytes per device call (a longer range is split at chunk boundaries)
DETECT_GUESS_MIN = 4096                # Reader.detect: events a call's first buffer holds at least, and one more per this many samples:
DETECT_GUESS_SAMPLES = 256             # a call that finds more says how many and is made once more
DECIMATE_CALL_BYTES = 1 << 30          # Reader.decimate: compressed bytes per device call (a longer range is split at output-row boundaries)
WAVEFORMS_CALL_BYTES = 1 << 30         # Reader.waveforms: compressed bytes per device call (a longer event list is split between events) ...
WAVEFORMS_OUT_BYTES = 1 << 30          # ... and the bytes of a call's result
MEAN_WAVEFORMS_EVENT_BYTES = 1 << 28   # Reader.mean_waveforms: the bytes of a call's event list (row, position, label and their order: 24 an event)
CORRELATE_CALL_BYTES = 1 << 30         # Reader.correlate: compressed bytes per device call (a longer range is split at chunk boundaries) ...
CORRELATE_OUT_BYTES = 1 << 30          # ... and the bytes of a call's result
TMATCH_CALL_BYTES = 1 << 30            # Reader.match_templates: compressed bytes per device call (a longer range is split at chunk boundaries)
TMATCH_GUESS_MIN = 4096                # Reader.match_templates: events a call's first buffer holds at least, and one more per this many samples:
TMATCH_GUESS_SAMPLES = 64              # a call that finds more says how many and is made once more
RESIDUAL_CALL_BYTES = 1 << 30          # Reader.residual: compressed bytes per device call (a longer range is split at chunk boundaries) ...
RESIDUAL_OUT_BYTES = 1 << 30           # ... and the bytes of a call's result
PROJECT_CALL_BYTES = 1 << 30          # Reader.project: compressed bytes per device call (a longer range is split at chunk boundaries) ...
PROJECT_OUT_BYTES = 1 << 30            # ... and the bytes of a call's result
WELCH_CALL_BYTES = 1 << 30             # Reader.welch: compressed bytes per device call (a longer range is split at group boundaries)
GRAM_CALL_BYTES = 1 << 30              # Reader.cov: compressed bytes per device call (a longer range is split at group boundaries)
GRAM_SLAB_BYTES = 1 << 30              # ... and partial results per call (one Gram matrix and one row of sums per group)
QUANTILE_CALL_BYTES = 1 << 30          # Reader.quantile / median / mad: compressed bytes per device call (split on chunk boundaries)
QUANTILE_SLAB_BYTES = 1 << 30          # ... and histogram bytes per call (2 KiB per window and column): the windows are scanned in runs
QUANTILE_METHODS = ('linear', 'lower', 'higher', 'nearest', 'midpoint')

logger = logging.getLogger('mtscomp_amd')
logger.setLevel(logging.INFO)
logger.addHandler(logging.NullHandler())

_seek_lock = Lock()


def add_default_handler(level='INFO', logger=logger):
    """Attach a stream handler (mtscomp.py:89-96)."""
    handler = logging.StreamHandler()
    handler.setLevel(level)
    handler.setFormatter(logging.Formatter('%(asctime)s [%(levelname).1s] %(message)s', '%H:%M:%S'))
    logger.addHandler(handler)


class Bunch(dict):
    """dict with attribute access (mtscomp.py:99-104)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


def _clip(x, lo, hi):
    return max(lo, min(hi, x))


# ------------------------------------------------------------------------------------------------
# config (mtscomp.py:176-209)
# ------------------------------------------------------------------------------------------------
def config_path():
    return (Path('~') / '.mtscomp').expanduser()


CONFIG_PATH = config_path()


def read_config(**kwargs):
    """Defaults < ~/.mtscomp < kwargs; None values are ignored (mtscomp.py:186-200)."""
    params = dict(DEFAULT_CONFIG)
    user = {}
    if CONFIG_PATH.exists():
        with CONFIG_PATH.open('r') as f:
            user = json.load(f)
    for layer in (user, kwargs):
        params.update({k: v for k, v in layer.items() if v is not None})
    return Bunch(params)


def write_config(**kwargs):
    """Merge kwargs into the user's configuration file and return what it now holds (mtscomp.py:203-209)."""
    merged = read_config(**kwargs)
    CONFIG_PATH.parent.mkdir(parents=True, exist_ok=True)
    CONFIG_PATH.write_text(json.dumps(merged, indent=2, sort_keys=True))
    return merged


# ------------------------------------------------------------------------------------------------
# raw I/O (mtscomp.py:115-140)
# ------------------------------------------------------------------------------------------------
def load_raw_data(path=None, n_channels=None, dtype=None, offset=None, mmap=True):
    """A flat binary file as an (n_samples, n_channels) array, memory mapped unless mmap=False (mtscomp.py:115-140).
    Contract: AssertionError for a missing file or dtype, ValueError when the size is no whole number of rows, an empty
    (0, n_channels) array for an empty file."""
    path = Path(path)
    assert path.exists(), "File %s does not exist." % path
    assert dtype, "The data type must be provided."
    n_channels, offset = n_channels or 1, offset or 0
    f_size = path.stat().st_size
    n_samples, rest = divmod(f_size - offset, np.dtype(dtype).itemsize * n_channels)
    if rest:
        raise ValueError(
            "The file size (%d bytes) is incompatible with the specified parameters "
            "(n_channels=%d, dtype=%s, offset=%d)" % (f_size, n_channels, dtype, offset))
    if n_samples <= 0:
        return np.zeros((0, n_channels), dtype=dtype)
    if not mmap:
        if offset > 0:  # pragma: no cover
            raise NotImplementedError()
        return np.fromfile(str(path), dtype).reshape((n_samples, n_channels))
    return np.memmap(str(path), dtype=dtype, shape=(n_samples, n_channels), offset=offset)


# ------------------------------------------------------------------------------------------------
# the codec (device side)
# ------------------------------------------------------------------------------------------------
def _one_block(chunks):
    """The chunks as one (rows, n_channels) array: a view when they already lie back to back in memory (consecutive
    slices of one memmap, the Writer's case), a concatenation otherwise."""
    if len(chunks) == 1:
        return chunks[0]
    first = chunks[0]
    if first.ndim == 2 and first.size and all(c.flags['C_CONTIGUOUS'] and c.dtype == first.dtype and c.shape[1:] == first.shape[1:]
                                              for c in chunks):
        addr = first.__array_interface__['data'][0]
        for c in chunks:
            if c.__array_interface__['data'][0] != addr:
                break
            addr += c.nbytes
        else:
            rows = sum(c.shape[0] for c in chunks)
            # (as_strided keeps `first`, hence the buffer under all the chunks, alive)
            return np.lib.stride_tricks.as_strided(first, shape=(rows,) + first.shape[1:], writeable=False)
    return np.concatenate(chunks, axis=0)


def decimate_taps(q):
    """scipy.signal.decimate's default FIR for factor q: firwin(20 * q + 1, 1 / q, window='hamming'), restated in numpy (a windowed
    sinc with cutoff 1/q of Nyquist, scaled to unit gain at DC)."""
    if not isinstance(q, (int, np.integer)) or isinstance(q, bool) or q < 2:
        raise ValueError("decimate_taps needs an int q >= 2, got %r" % (q,))
    n = 20 * int(q) + 1
    f = 1.0 / int(q)
    m = np.arange(n) - (n - 1) / 2.0
    h = f * np.sinc(f * m)
    h *= 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))
    return h / h.sum()


def highpass_taps(cutoff_hz, sample_rate, n_taps=101):
    """scipy.signal.firwin(n_taps, cutoff_hz, pass_zero=False, fs=sample_rate) restated in numpy: a Hamming-windowed high-pass of odd
    length, scaled to unit gain at Nyquist.  The spike band of Reader.detect is highpass_taps(300, sample_rate)."""
    if not isinstance(n_taps, (int, np.integer)) or isinstance(n_taps, bool) or n_taps < 3 or n_taps % 2 == 0:
        raise ValueError("highpass_taps needs an odd int n_taps >= 3, got %r" % (n_taps,))
    try:
        cutoff, rate = float(cutoff_hz), float(sample_rate)
    except (TypeError, ValueError):
        raise ValueError("cutoff_hz and sample_rate must be numbers") from None
    if not (np.isfinite(rate) and rate > 0 and 0 < cutoff < rate / 2):
        raise ValueError("highpass_taps needs 0 < cutoff_hz < sample_rate / 2, got %r and %r" % (cutoff_hz, sample_rate))
    n = int(n_taps)
    m = np.arange(n) - (n - 1) / 2.0
    f = 2.0 * cutoff / rate
    h = np.sinc(m) - f * np.sinc(f * m)
    h *= 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))
    return h / (h * np.cos(np.pi * m)).sum()


def welch_window(window, nperseg):
    """The taper of Reader.welch: 'hann', 'hamming' or 'boxcar' as the periodic windows of scipy.signal.get_window(window, nperseg)
    (restated in numpy), or a 1-D array of nperseg finite numbers, as float64."""
    if isinstance(window, str):
        n = np.arange(nperseg)
        if window == 'hann':
            return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / nperseg)
        if window == 'hamming':
            return 0.54 - 0.46 * np.cos(2.0 * np.pi * n / nperseg)
        if window == 'boxcar':
            return np.ones(nperseg)
        raise ValueError("window must be 'hann', 'hamming', 'boxcar' or an array, got %r" % (window,))
    w = np.asarray(window, dtype=np.float64)
    if w.ndim != 1 or w.size != nperseg or not np.isfinite(w).all():
        raise ValueError("a window array must hold nperseg = %d finite numbers" % nperseg)
    return w


def _float_dtype(dtype):
    """The compute type of Reader.decimate / welch: float32 or float64 as a numpy dtype."""
    try:
        dt = np.dtype(dtype)
    except TypeError:
        raise ValueError("dtype must be float32 or float64, got %r" % (dtype,))
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("dtype must be float32 or float64, got %r" % (dtype,))
    return dt


def _fir_taps(taps):
    """The taps of Reader.decimate / detect as a float64 array: 1 to hip.DECIMATE_MAX_TAPS finite numbers."""
    taps = np.asarray(taps, dtype=np.float64)
    if taps.ndim != 1 or not 1 <= taps.size <= hip.DECIMATE_MAX_TAPS or not np.isfinite(taps).all():
        raise ValueError("taps must be a 1-D sequence of 1 to %d finite numbers" % hip.DECIMATE_MAX_TAPS)
    return taps


def whitening_weights(cov, eps=0.0):
    """The symmetric float64 ZCA whitening matrix E diag(1 / sqrt(max(lambda, 0) + eps)) E^T of a covariance matrix, from
    np.linalg.eigh(cov).  With c = r.cov(), r.project(whitening_weights(c.cov[0], eps), offset=c.mean[0]) is the whitened recording.
    ValueError for a matrix that is not square or not finite, a negative or non-finite eps, or a singular matrix with eps == 0."""
    c = np.asarray(cov, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or not c.shape[0]:
        raise ValueError("cov must be a square matrix, got shape %r" % (c.shape,))
    if not np.isfinite(c).all():
        raise ValueError("cov must be finite")
    if not isinstance(eps, (int, float, np.integer, np.floating)) or isinstance(eps, bool) or not np.isfinite(eps) or eps < 0:
        raise ValueError("eps must be a finite number >= 0, got %r" % (eps,))
    lam, vec = np.linalg.eigh(0.5 * (c + c.T))
    d = np.maximum(lam, 0.0) + float(eps)
    if d.min() <= 0 or (eps == 0 and d.min() <= d.max() * np.finfo(np.float64).eps * c.shape[0]):
        raise ValueError("cov is singular (smallest eigenvalue %g): pass eps > 0" % lam.min())
    w = (vec / np.sqrt(d)) @ vec.T
    return 0.5 * (w + w.T)


def waveform_basis(waveforms, n_components=3):
    """The temporal basis of Reader.waveform_features from snippets: the n_components leading eigenvectors of the temporal Gram
    matrix, as float32 (P, T).  waveforms: any (..., T, W) array of numbers -- the snippets of Reader.waveforms, or the mean of
    Reader.mean_waveforms; every column (..., :, w) is one T-vector v, and a column that holds a NaN is dropped.  G = sum v v^T in
    float64, not centred (as Kilosort does); np.linalg.eigh(G); the eigenvectors of the P largest eigenvalues in descending order,
    each signed so that its entry of largest magnitude (the first on a tie) is positive.  ValueError for an array of fewer than
    two axes, an n_components that is not an int in [1, T], or fewer than n_components columns without a NaN."""
    w = np.asarray(waveforms)
    if w.ndim < 2 or w.dtype.kind not in 'fiu' or not w.shape[-2]:
        raise ValueError("waveforms must be a (..., T, W) array of numbers")
    T = int(w.shape[-2])
    if not isinstance(n_components, (int, np.integer)) or isinstance(n_components, bool) or not 1 <= n_components <= T:
        raise ValueError("n_components must be an int in [1, %d], got %r" % (T, n_components))
    P = int(n_components)
    cols = np.moveaxis(w, -2, -1).reshape(-1, T)                      # one column a row
    gram, kept = np.zeros((T, T), np.float64), 0
    for a in range(0, cols.shape[0], 1 << 16):                        # (float64 copies of 2^16 columns at a time)
        v = cols[a:a + (1 << 16)].astype(np.float64)
        v = v[~np.isnan(v).any(axis=1)]
        if not np.isfinite(v).all():
            raise ValueError("waveforms must be finite or NaN")
        gram += v.T @ v
        kept += v.shape[0]
    if kept < P:
        raise ValueError("%d components need at least as many columns without a NaN, got %d" % (P, kept))
    _, vec = np.linalg.eigh(gram)                                     # (ascending eigenvalues)
    basis = vec[:, ::-1][:, :P].T.astype(np.float32)
    top = np.abs(basis).argmax(axis=1)                                # (the first of equal magnitudes, as float32)
    return np.ascontiguousarray(basis * np.where(basis[np.arange(P), top] < 0, np.float32(-1), np.float32(1))[:, None])


_DETECT_CAP_AT = 11                     # where max_events stands among the op's own arguments of codec.detect ...
_TMATCH_CAP_AT = 11                     # ... and of codec.match_templates / match_residual (the subtracted events follow it)


def _templates32(templates):
    """templates as a C-contiguous float32 (K, T, W) array, and whether one 2-D (T, W) template was given."""
    k = np.asarray(templates)
    if k.dtype.kind not in 'fiu' or k.ndim not in (2, 3):
        raise ValueError("templates must be a (K, T, W) or (T, W) array of numbers")
    with np.errstate(over='ignore'):
        return np.ascontiguousarray((k[None] if k.ndim == 2 else k).astype(np.float32)), k.ndim == 2


def _template_args(templates, before, cols, op):
    """The templates and `before` of Reader.correlate / match_templates / residual (`op`, for the messages) on the columns `cols`
    -> (the float32 (K, T, W) templates, whether one 2-D template was given, before as an int)."""
    k, squeeze = _templates32(templates)
    n_out, T, W = k.shape
    if W != cols.size:
        raise ValueError("templates have %d columns for %d selected channels" % (W, cols.size))
    if not 1 <= W <= hip.CORRELATE_MAX_COLS:
        raise ValueError("%s takes 1 to %d columns, got %d" % (op, hip.CORRELATE_MAX_COLS, W))
    if not 1 <= T <= hip.CORRELATE_MAX_T:
        raise ValueError("templates have 1 to %d rows, got %d" % (hip.CORRELATE_MAX_T, T))
    if not 1 <= n_out <= hip.CORRELATE_MAX_OUT:
        raise ValueError("%s takes 1 to %d templates, got %d" % (op, hip.CORRELATE_MAX_OUT, n_out))
    if not isinstance(before, (int, np.integer)) or isinstance(before, bool) or not 0 <= before <= T:
        raise ValueError("before must be an int in [0, %d], got %r" % (T, before))
    if not np.isfinite(k).all():
        raise ValueError("templates must be finite in float32")
    return k, squeeze, int(before)


def _event_arrays(found):
    """The (row, index, value) arrays of the parts of detect / match_templates, in order, as one int64, int64 and float32 array."""
    return tuple(np.concatenate([f[j] for f in found]).astype(t) if found else np.zeros(0, t)
                 for j, t in enumerate((np.int64, np.int64, np.float32)))


def _again_with_room(cap_at):
    """The `again` of _halo_parts for detect / match_templates: a part whose buffer (args[cap_at] events) was short is sent once more
    with room for all the events it counted."""
    def again(out, args):
        if out[1] > args[cap_at] and all(v == hip.CHUNK_OK for v in out[0]):
            return args[:cap_at] + (out[1],) + args[cap_at + 1:]
    return again


def template_amplitudes(score, template, templates):
    """The least-squares amplitudes of matched templates: score[e] / sum(templates[template[e]] ** 2) -- the a that minimises
    |z - a * K| when score is the matched filter's <z, K>.  The norms are summed in float64 from the templates rounded to float32 (what
    the device multiplies by), the quotient is formed in float64 and rounded once to float32.  score, template: the arrays of a
    match_templates result (or any of one shape); templates: (K, T, W), or (T, W) for one.  With ev = r.match_templates(K, thr),
    r.match_templates(K, thr, subtract=(ev.sample, ev.template, template_amplitudes(ev.score, ev.template, K))) is the second pass of
    a template-matching sorter.  ValueError for an index outside the templates or a template of zero norm."""
    k, _ = _templates32(templates)
    if not np.isfinite(k).all():
        raise ValueError("templates must be finite in float32")
    sc, tp = np.asarray(score), np.asarray(template)
    if sc.dtype.kind not in 'fiu' or (tp.size and tp.dtype.kind not in 'iu') or sc.shape != tp.shape:
        raise ValueError("score (numbers) and template (ints) must have one shape")
    tp = tp.astype(np.int64)
    if tp.size and not (0 <= tp.min() and tp.max() < k.shape[0]):
        raise ValueError("template indices must lie in [0, %d)" % k.shape[0])
    norm = (k.astype(np.float64) ** 2).reshape(k.shape[0], -1).sum(axis=1)
    if tp.size and not (norm[tp] > 0).all():
        raise ValueError("template %d has zero norm" % int(tp[norm[tp] <= 0].ravel()[0]))
    with np.errstate(over='ignore'):
        return (sc.astype(np.float64) / norm[tp]).astype(np.float32)


def _sub_events(sample, template, amplitude, n_templates, n_samples):
    """The events of Reader.residual / match_templates(subtract=) as (sample int64, template int32, amplitude float32), stable-sorted by
    sample: three 1-D arrays of one length, 0 <= sample < n_samples, 0 <= template < n_templates, amplitudes finite in float32."""
    sm, tp, am = np.asarray(sample), np.asarray(template), np.asarray(amplitude)
    if sm.ndim != 1 or tp.ndim != 1 or am.ndim != 1 or not sm.size == tp.size == am.size:
        raise ValueError("the subtracted events are three 1-D arrays of one length: sample, template, amplitude")
    if sm.size > hip.RESIDUAL_MAX_EVENTS:
        raise ValueError("at most %d subtracted events, got %d" % (hip.RESIDUAL_MAX_EVENTS, sm.size))
    if sm.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
    if sm.dtype.kind not in 'iu' or tp.dtype.kind not in 'iu' or am.dtype.kind not in 'fiu':
        raise ValueError("sample and template must be ints and amplitude numbers")
    if sm.min() < 0 or sm.max() >= n_samples:
        raise ValueError("subtracted samples must lie in [0, %d)" % n_samples)
    if tp.min() < 0 or tp.max() >= n_templates:
        raise ValueError("subtracted template indices must lie in [0, %d)" % n_templates)
    with np.errstate(over='ignore'):
        am = am.astype(np.float32)
    if not np.isfinite(am).all():
        raise ValueError("subtracted amplitudes must be finite in float32")
    order = np.argsort(sm, kind='stable')
    return np.ascontiguousarray(sm.astype(np.int64)[order]), np.ascontiguousarray(tp.astype(np.int32)[order]), np.ascontiguousarray(am[order])


def _window_rows(window, i0, i1):
    """The window of Reader.window_stats / quantile / cov over rows [i0, i1) as an int: None is one window over the range."""
    if window is None:
        window = max(i1 - i0, 1)
    if not isinstance(window, (int, np.integer)) or isinstance(window, bool) or window < 1:
        raise ValueError("window must be an int >= 1 or None, got %r" % (window,))
    return int(window)


def _lane_reduction(name):
    """HipCodec.<name>(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, <the op's own arguments>, lane=None):
    hip.<name> (looked up when called) on the device of `lane` (modulo the devices, default the first) -> what it returns."""
    def call(self, cache_id, *args, lane=None):
        return getattr(hip, name)(cache_id or 0, *args, device=self.devices[(lane or 0) % len(self.devices)])
    call.__name__, call.__qualname__ = name, 'HipCodec.' + name
    call.__doc__ = ("mts_%s for the chunks `keys` on one device; cache_id: the lane's decoded-chunk cache (0: none), chunks with "
                    "lens[i] == 0 are read there (hip.%s)." % (name, name))
    return call


class HipCodec:
    """Per-chunk codec on MI355X.  ``devices``: list of device indices (default: all visible)."""

    name = 'hip'
    takes_ranges = True          # decompress() also accepts (buffer, offsets, lengths)

    def __init__(self, devices=None):
        n = hip.require_device()
        self.devices = list(range(n)) if devices is None else [int(d) for d in devices]
        assert self.devices and all(0 <= d < n for d in self.devices), "invalid device list"
        self._pool = None                       # one host thread per entry of `devices`, kept for the codec's lifetime
        self._pool_lock = threading.Lock()

    # -- transforms alone (diff_along_axis / cumsum_along_axis)
    def delta(self, arr, flags):
        return hip.delta_transpose(arr, flags, device=self.devices[0])

    def cumsum(self, stream, nt, nc, dtype, flags):
        return hip.cumsum_transpose(stream, nt, nc, dtype, flags, device=self.devices[0])

    def _shards(self, n):
        g = len(self.devices)
        return [list(range(k, n, g)) for k in range(g)] if g > 1 and n > 1 else [list(range(n))]

    def compress(self, chunks, flags, level=6):
        """chunks: list of (n_t, n_c) arrays -> list of zlib streams (order preserved)."""
        n = len(chunks)
        out = [None] * n
        shards = [s for s in self._shards(n) if s]

        def run(k):
            ids = shards[k]
            rows = [chunks[i].shape[0] for i in ids]
            data = _one_block([chunks[i] for i in ids])
            bounds = np.concatenate(([0], np.cumsum(rows)))
            res = hip.compress_chunks(data, bounds, flags, level, device=self.devices[k % len(self.devices)])
            for i, b in zip(ids, res):
                out[i] = b
        self.run_lanes(run, len(shards))
        return out

    takes_out = True

    def decompress(self, cbufs, n_rows, n_channels, dtype, flags, out=None, lane=None):
        """-> (status list, list of (n_rows[i], n_channels) arrays or None).  `out`: optional array of exactly the decoded
        size, filled in place when one device does the whole call: a codec with one device, or `lane` = the entry of
        `devices` (modulo their number) that is to take all of it -- Reader.tofile hands its pieces to the devices in turn."""
        one = self.devices[lane % len(self.devices)] if lane is not None else self.devices[0] if len(self.devices) == 1 else None
        if isinstance(cbufs, tuple):                        # (buffer, offsets, lengths): chunks already in one buffer
            buf, offs, lens = cbufs
            if one is not None:
                return hip.decompress_chunks(cbufs, n_rows, n_channels, dtype, flags, device=one, out=out)
            mv = memoryview(buf)
            cbufs = [mv[o:o + l] for o, l in zip(offs, lens)]
        elif one is not None:
            return hip.decompress_chunks(cbufs, n_rows, n_channels, dtype, flags, device=one, out=out)
        n = len(cbufs)
        status, arrays = [0] * n, [None] * n
        shards = [s for s in self._shards(n) if s]

        def run(k):
            ids = shards[k]
            st, arrs = hip.decompress_chunks([cbufs[i] for i in ids], [n_rows[i] for i in ids], n_channels, dtype,
                                             flags, device=self.devices[k % len(self.devices)])
            for i, s, a in zip(ids, st, arrs):
                status[i], arrays[i] = s, a
        self.run_lanes(run, len(shards))
        return status, arrays

    # -- decoded-chunk cache in HBM (Reader random access): one cache per lane, chunk k lives on lane k mod n_lanes
    device_cache = True
    leading_channels = True      # cache_read_slices(..., n_leading=): chunks decoded up to the leading channels a request needs

    @property
    def n_lanes(self):
        return len(self.devices)

    def cache_create(self, capacity_bytes, lane=0):
        return hip.cache_create(capacity_bytes, device=self.devices[lane % len(self.devices)])

    # page-locked host memory (Reader.tofile's pieces, the compressed bytes of slices): from a pool that outlives the call
    host_buffer = staticmethod(hip.HostBuffer)
    host_buffer_take = staticmethod(hip.pinned_pool.take)
    host_buffer_give = staticmethod(hip.pinned_pool.give)

    # the device reductions of the Reader, one call for the chunks of one lane
    window_stats, rank_hist, decimate, detect, welch, gram = map(
        _lane_reduction, ('window_stats', 'rank_hist', 'decimate', 'detect', 'welch', 'gram'))
    project = _lane_reduction('project')
    waveforms = _lane_reduction('waveforms')
    mean_waveforms = _lane_reduction('mean_waveforms')
    waveform_features = _lane_reduction('waveform_features')
    localize = _lane_reduction('localize')
    correlate = _lane_reduction('correlate')
    match_templates = _lane_reduction('match_templates')
    residual = _lane_reduction('residual')
    match_residual = _lane_reduction('match_residual')
    filtered_rank_hist = _lane_reduction('filtered_rank_hist')
    filtered_gram = _lane_reduction('filtered_gram')

    cache_destroy = staticmethod(hip.cache_destroy)
    cache_query = staticmethod(hip.cache_query)
    cache_read_rows = staticmethod(hip.cache_read_rows)
    cache_read_slices = staticmethod(hip.cache_read_slices)

    def run_lanes(self, fn, n):
        """fn(0) ... fn(n - 1), each on a host thread of its own (ctypes releases the GIL): the threads are the codec's, made on
        first use and kept -- a ThreadPool per call cost a thread start and a join per device and call."""
        if n <= 1:
            if n:
                fn(0)
            return
        with self._pool_lock:
            if self._pool is None or self._pool_size < n:
                if self._pool is not None:
                    self._pool.close()
                self._pool_size = max(n, len(self.devices))
                self._pool = ThreadPool(self._pool_size)
            pool = self._pool
        pool.map(fn, range(n), chunksize=1)

    def close(self):
        """Ends the lane threads and frees the page-locked buffers the process-wide pool keeps idle for Reader.tofile and the
        slice reads (hip.pinned_pool: up to MTSCOMP_PINNED_KEEP_MB, default 2 GiB, would stay pinned otherwise)."""
        with self._pool_lock:
            if self._pool is not None:
                self._pool.close()
                self._pool = None
        hip.pinned_pool.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


_default_codec = None


def get_codec():
    """The process-wide device codec (created on first use; raises without library/GPU)."""
    global _default_codec
    if _default_codec is None:
        _default_codec = HipCodec()
    return _default_codec


def set_codec(codec):
    """Install a codec object (tests inject the CPU oracle here to exercise the host logic without a
    GPU; the package itself never constructs anything but ``HipCodec``)."""
    global _default_codec
    _default_codec = codec


def _int_flags(do_time_diff, do_spatial_diff, chunk_order):
    return hip.make_flags(bool(do_time_diff), bool(do_spatial_diff), chunk_order)


def diff_along_axis(chunk, axis=None):
    """np.diff along `axis` keeping the first row/column (mtscomp.py:143-159)."""
    if axis is None:
        return chunk
    assert 0 <= axis < chunk.ndim
    hip.check_dtype(chunk.dtype)
    flags = hip.FLAG_TIME_DIFF if axis == 0 else hip.FLAG_SPATIAL_DIFF
    chunk = np.ascontiguousarray(chunk)
    out = get_codec().delta(chunk, flags)          # order 'C': same layout as the input
    return out.view(chunk.dtype).reshape(chunk.shape)


def cumsum_along_axis(chunk, axis=None):
    """Inverse of diff_along_axis (mtscomp.py:162-169)."""
    if axis is None:
        return chunk
    assert 0 <= axis < chunk.ndim
    hip.check_dtype(chunk.dtype)
    flags = hip.FLAG_TIME_DIFF if axis == 0 else hip.FLAG_SPATIAL_DIFF
    chunk = np.ascontiguousarray(chunk)
    return get_codec().cumsum(chunk, chunk.shape[0], chunk.shape[1], chunk.dtype, flags)


# ------------------------------------------------------------------------------------------------
# Writer (mtscomp.py:216-511)
# ------------------------------------------------------------------------------------------------
class Writer:
    """Compress a raw data file chunk by chunk.

    Keyword arguments as in the reference (chunk_duration, algorithm, comp_level, do_time_diff,
    do_spatial_diff, n_threads, before_check, check_after_compress, chunk_order) plus
    ``batch_chunks`` (chunks per device call) and ``codec`` (defaults to the MI355X codec).
    """

    # configuration keys a Writer keeps as attributes of the same name
    _CONFIG_ATTRS = ('chunk_duration', 'algorithm', 'comp_level', 'do_time_diff', 'do_spatial_diff', 'n_threads',
                     'check_after_compress', 'chunk_order')

    def __init__(self, before_check=None, codec=None, **kwargs):
        self.pool = None
        self.quiet = kwargs.pop('quiet', False)
        self.config = read_config(**kwargs)
        for key in self._CONFIG_ATTRS:
            setattr(self, key, self.config[key])
        assert self.algorithm == 'zlib', "Only zlib is currently supported."
        self.before_check = before_check if before_check is not None else (lambda x: None)
        self.batch_chunks = int(self.config.get('batch_chunks', None) or DEFAULT_BATCH_CHUNKS)
        self._codec = codec

    @property
    def codec(self):
        return self._codec or get_codec()

    def _need(self, given, key, message):
        """A parameter from the call or the configuration; ValueError(message) when neither has it."""
        value = given or self.config.get(key, None)
        if not value:
            raise ValueError(message)
        return value

    def open(self, data_path, sample_rate=None, n_channels=None, dtype=None, offset=None, mmap=True):
        """Open the raw file and lay out the chunks (mtscomp.py:257-322).  A .npy file brings its own shape and dtype
        (arrays of 3 and more dimensions are flattened to (-1, last axis), the header keeps the original shape); a flat file
        needs n_channels and dtype.  ValueError for a missing sample rate / n_channels / dtype, AssertionError for no data."""
        self.data_path = Path(data_path)
        sample_rate = self._need(sample_rate, 'sample_rate', "Please provide a sample rate (-s option in the command-line).")
        if str(data_path).endswith('.npy'):
            data = np.load(data_path, mmap_mode='r')
            self.shape = data.shape
            self.data = data if data.ndim < 3 else np.reshape(data, (-1, data.shape[-1]))
            self.dtype = self.data.dtype
            n_channels = self.data.shape[1]
        else:
            n_channels = self._need(n_channels, 'n_channels', "Please provide n_channels (-n option in the command-line).")
            self.dtype = np.dtype(self._need(dtype, 'dtype', "Please provide a dtype (-d option in the command-line)."))
            self.data = load_raw_data(data_path, n_channels=n_channels, dtype=self.dtype)
            self.shape = self.data.shape
        assert sample_rate > 0 and n_channels > 0
        assert self.data.ndim == 2
        self.sample_rate = float(sample_rate)
        self.n_samples, self.n_channels = self.data.shape
        assert self.n_samples > 0 and self.n_channels > 0
        assert self.n_channels == n_channels
        self.file_size = self.data.size * self.data.itemsize
        logger.info("Opening %s, duration %.1fs, %d channels.", data_path, self.n_samples / self.sample_rate, self.n_channels)
        self._compute_chunk_bounds()
        self.sha1_compressed, self.sha1_uncompressed = hashlib.sha1(), hashlib.sha1()

    def _compute_chunk_bounds(self):
        """mtscomp.py:324-339 (np.round: half to even)."""
        chunk_size = int(np.round(self.chunk_duration * self.sample_rate))
        bounds = list(range(0, self.n_samples, chunk_size))
        if bounds[-1] < self.n_samples:
            bounds.append(self.n_samples)
        self.chunk_bounds = bounds
        self.n_chunks = len(bounds) - 1
        assert bounds[0] == 0 and bounds[-1] == self.n_samples
        # A batch is what one round of device calls processes (the reference: one chunk per thread).
        self.batch_size = max(1, self.batch_chunks * max(1, len(getattr(self.codec, 'devices', [0]))))
        self.n_batches = int(np.ceil(self.n_chunks / self.batch_size))

    def get_cmeta(self):
        """The .ch header (mtscomp.py:341-358): same keys, same value types."""
        return {
            'version': FORMAT_VERSION,
            'algorithm': self.algorithm,
            'comp_level': self.comp_level,
            'do_time_diff': self.do_time_diff,
            'do_spatial_diff': self.do_spatial_diff,
            'dtype': str(np.dtype(self.dtype)),
            'n_channels': self.n_channels,
            'sample_rate': self.sample_rate,
            'chunk_bounds': self.chunk_bounds,
            'chunk_offsets': self.chunk_offsets,
            'chunk_order': self.chunk_order,
            'sha1_compressed': self.sha1_compressed.hexdigest(),
            'sha1_uncompressed': self.sha1_uncompressed.hexdigest(),
            'shape': self.shape,
        }

    def get_chunk(self, chunk_idx):
        """mtscomp.py:360-373."""
        assert 0 <= chunk_idx <= self.n_chunks - 1
        return self.data[self.chunk_bounds[chunk_idx]:self.chunk_bounds[chunk_idx + 1], :]

    def _compress_chunk(self, chunk_idx):
        """(chunk_idx, (raw chunk, compressed bytes)) -- mtscomp.py:375-397; a device batch of one."""
        return chunk_idx, self.compress_batch(chunk_idx, chunk_idx + 1)[chunk_idx]

    def compress_batch(self, first_chunk, last_chunk):
        """Chunks [first_chunk, last_chunk) -> {idx: (raw chunk, compressed bytes)}
        (mtscomp.py:399-423; the per-chunk work of :375-397 happens on the device)."""
        assert 0 <= first_chunk < last_chunk <= self.n_chunks
        ids = list(range(first_chunk, last_chunk))
        chunks = [self.get_chunk(i) for i in ids]
        flags = _int_flags(self.do_time_diff, self.do_spatial_diff, self.chunk_order)
        # the reference never forwards comp_level to zlib (mtscomp.py:394): level 6 always
        cbufs = self.codec.compress(chunks, flags, 6)
        return {i: (c, b) for i, c, b in zip(ids, chunks, cbufs)}

    def write(self, out, outmeta):
        """Write .cbin + .ch; returns csize / raw size (mtscomp.py:425-507)."""
        if not out:
            out = self.data_path.with_suffix('.c' + self.data_path.suffix[1:])
        if not outmeta:
            outmeta = self.data_path.with_suffix('.ch')
        Path(out).parent.mkdir(exist_ok=True, parents=True)
        self.chunk_offsets = [0]
        logger.info("Starting compression on %s.", getattr(self.codec, 'name', 'codec'))
        # The two SHA-1s and the file write are host work in file order (mtscomp.py:477-483).  One SHA-1 over the whole raw
        # file (~1.2 GB/s per core) is the slowest thing in a file-to-file run, so it gets its own thread from the start
        # (it needs nothing from the devices: hashing chunk after chunk is hashing the file); a second thread writes and
        # hashes the compressed chunks of the previous batch while the devices work on the next one (hashlib and ctypes
        # release the GIL).
        state = {'offset': 0}

        def hash_raw():
            for idx in range(self.n_chunks):
                self.sha1_uncompressed.update(np.ascontiguousarray(self.get_chunk(idx)))

        def consume(done):
            for idx in sorted(done.keys()):                     # strictly in file order
                _, cbuf = done[idx]
                fb.write(cbuf)
                state['offset'] += len(cbuf)
                self.chunk_offsets.append(state['offset'])
                self.sha1_compressed.update(cbuf)

        with open(out, 'wb') as fb, ThreadPool(2) as sink:
            raw_job = sink.apply_async(hash_raw)
            pending = None
            for batch in range(self.n_batches):
                first = self.batch_size * batch
                last = min(self.batch_size * (batch + 1), self.n_chunks)
                done = self.compress_batch(first, last)
                assert set(done.keys()) <= set(range(first, last))
                if pending is not None:
                    pending.get()                               # keep at most one batch in flight behind the devices
                pending = sink.apply_async(consume, (done,))
            if pending is not None:
                pending.get()
            raw_job.get()
            csize = fb.tell()
        assert self.chunk_offsets[-1] == csize
        ratio = csize / self.file_size
        logger.info("Wrote %s (%.1f GB, -%.3f%%).", out, csize / 1024 ** 3, 100 - 100 * ratio)
        with open(outmeta, 'w') as f:
            json.dump(self.get_cmeta(), f, indent=2, sort_keys=True)
        if self.check_after_compress:
            self.before_check(self)
            try:
                check(self.data, out, outmeta, codec=self._codec)
            except AssertionError:
                raise RuntimeError(
                    "CRITICAL ERROR: automatic check failed when compressing the data. "
                    "Report immediately to " + CRITICAL_ERROR_URL)
            logger.debug("Automatic integrity check after compression PASSED.")
        return ratio

    def close(self):
        """mtscomp.py:509-511."""
        mm = getattr(self.data, '_mmap', None)
        if mm is not None:
            mm.close()


# ------------------------------------------------------------------------------------------------
# Reader (mtscomp.py:514-859)
# ------------------------------------------------------------------------------------------------
def _join_rows(chunks):
    """np.concatenate(chunks, axis=0) -- without the copy when the chunks already lie back to back in memory
    (the arrays of one codec call do)."""
    if len(chunks) == 1:
        return chunks[0]
    addr = [c.__array_interface__['data'][0] for c in chunks]
    if all(c.flags.c_contiguous and c.dtype == chunks[0].dtype and c.shape[1] == chunks[0].shape[1] for c in chunks) and \
            all(addr[k] + chunks[k].nbytes == addr[k + 1] for k in range(len(chunks) - 1)) and \
            all(c.base is not None and c.base is chunks[0].base for c in chunks):
        total = sum(c.shape[0] for c in chunks)
        return np.lib.stride_tricks.as_strided(chunks[0], shape=(total, chunks[0].shape[1]))
    return np.concatenate(chunks, axis=0)


def _unlink_lazily(path):
    """path.unlink() whose page-cache work happens off the caller's thread: the name is gone on return (a new file of that name
    is a new file), the old file's pages -- a few hundred thousand of them for a recording on a RAM-backed file system, freed one
    by one when its last reference goes -- are released by a thread that only closes a descriptor."""
    try:
        fd = os.open(str(path), os.O_RDONLY)
    except OSError:
        Path(path).unlink()
        return
    try:
        Path(path).unlink()
    finally:
        threading.Thread(target=os.close, args=(fd,), daemon=True).start()


class Reader:
    """NumPy-style read access to a compressed file; chunks are decoded on the device."""

    def __init__(self, codec=None, **kwargs):
        self.pool = None
        self.cdata = None
        self.quiet = kwargs.pop('quiet', False)
        self.config = read_config(**kwargs)
        self.cache_size = self.config.cache_size
        self.check_after_decompress = self.config.check_after_decompress
        self.batch_chunks = int(self.config.get('batch_chunks', None) or DEFAULT_BATCH_CHUNKS)
        # partial_decode=True (off by default): Reader[rows, :k] may inflate only the prefix of a chunk's stream its leading
        # channels need.  The reference inflates -- and adler32-checks -- the whole chunk on every read (mtscomp.py:618-621);
        # a prefix decode cannot, so it is the caller's explicit choice.
        self.partial_decode = bool(self.config.get('partial_decode', False))
        self._codec = codec
        self._cache = OrderedDict()
        self._dev_caches = None                                   # decoded-chunk caches in HBM, one per lane of the codec (chunk k -> lane k mod lanes)
        self._dev_cache_lock = threading.Lock()
        self._cache_lock = threading.RLock()                      # the host LRU is shared by the threads that slice (mtscomp.py:648)
        self._dev_cache_bytes = int(float(os.environ.get('MTSCOMP_DEVICE_CACHE_GB', DEFAULT_DEVICE_CACHE_GB)) * 2 ** 30)
        self._pin = None                                          # page-locked buffer the compressed bytes of slices are read into
        self._ra, self._ra_calls, self._ra_pending = 1, 0, {}     # read-ahead of the device cache (see _read_ahead)
        self._ra_lock = threading.Lock()                          # (slices may come from several threads)
        self._pin_lock = threading.Lock()
        self._map_lock = threading.Lock()
        self._cmap = self._cmap_view = None
        self._cmap_size = -1
        self._io_pool = None

    @property
    def codec(self):
        return self._codec or get_codec()

    # header fields a Reader keeps as attributes of the same name
    _HEADER_ATTRS = ('n_channels', 'sample_rate', 'chunk_offsets', 'chunk_bounds', 'chunk_order')

    def open(self, cdata, cmeta=None):
        """Attach a compressed file (path or open binary file object) and its header: a dict, a path, or -- by default --
        the .ch file next to a .cbin path (mtscomp.py:536-580)."""
        header = cmeta if cmeta is not None else Path(cdata).with_suffix('.ch')
        if not isinstance(header, dict):
            header = json.loads(Path(header).read_text())
        assert isinstance(header, dict)
        self.cmeta = Bunch(header)
        for key in self._HEADER_ATTRS:
            setattr(self, key, self.cmeta[key])
        self.dtype = np.dtype(self.cmeta.dtype)
        self.n_chunks = len(self.chunk_bounds) - 1
        self.n_samples = self.chunk_bounds[-1]
        self.shape, self.ndim = (self.n_samples, self.n_channels), 2
        self.batch_size = max(1, self.batch_chunks * max(1, len(getattr(self.codec, 'devices', [0]))))
        self.n_batches = int(np.ceil(self.n_chunks / self.batch_size))
        if isinstance(cdata, (str, Path)):
            if Path(cdata).suffix in ('.bin', '.dat'):  # pragma: no cover
                logger.error("File to decompress has unexpected extension %s.", Path(cdata).suffix)
            cdata = open(cdata, 'rb')
        self.cdata = cdata
        self.set_cache_size()

    def set_cache_size(self, cache_size=None):
        """LRU size for decoded chunks (mtscomp.py:582-588)."""
        cache_size = cache_size or self.cache_size
        assert cache_size > 0
        with self._cache_lock:
            self.cache_size = cache_size
            while len(self._cache) > self.cache_size:
                self._cache.popitem(last=False)

    def iter_chunks(self, first_chunk=0, last_chunk=None):
        """Yield (chunk_idx, chunk_start, chunk_length) (mtscomp.py:590-600)."""
        last_chunk = last_chunk if last_chunk is not None else self.n_chunks - 1
        for idx in range(first_chunk, last_chunk + 1):
            yield idx, self.chunk_offsets[idx], self.chunk_offsets[idx + 1] - self.chunk_offsets[idx]

    def _pread(self, length, start):
        if hasattr(os, 'pread'):
            buf = os.pread(self.cdata.fileno(), length, start)       # thread safe (mtscomp.py:609)
            if len(buf) < length:                                    # one pread returns at most 2 GiB - 4 KiB on Linux
                parts = [buf]
                got = len(buf)
                while got < length:
                    more = os.pread(self.cdata.fileno(), length - got, start + got)
                    if not more:
                        break
                    parts.append(more)
                    got += len(more)
                buf = b''.join(parts)
        else:  # pragma: no cover
            with _seek_lock:
                self.cdata.seek(start)
                buf = self.cdata.read(length)
        assert len(buf) == length
        return buf

    def _map_range(self, length, start):
        """`length` bytes at `start` of the compressed file as a uint8 view of a read-only MAPPING of the file: no read call and no
        copy on this side -- the library's host threads copy the bytes out of the page cache into its page-locked pieces while
        the DMA of the piece before runs (mts_cache_*: staged copies).  A cold window's two chunks were 1.1 ms of preadv on eight
        Python threads plus 0.65 ms of DMA before (round 6).  None when the file cannot be mapped, or the range is not inside it
        (the caller's pread then fails the way the reference's does, mtscomp.py:609-612)."""
        if not MAP_CDATA or length <= 0:
            return None
        try:
            with self._map_lock:
                size = os.fstat(self.cdata.fileno()).st_size
                if start + length > size:
                    return None
                if self._cmap is None or self._cmap_size != size:
                    import mmap
                    self._cmap_view = None
                    if self._cmap is not None:
                        try:
                            self._cmap.close()
                        except (BufferError, ValueError):
                            pass                                     # (a view of the old mapping is still out: it goes with its last user)
                    self._cmap = mmap.mmap(self.cdata.fileno(), 0, access=mmap.ACCESS_READ)
                    self._cmap_size = size
                    self._cmap_view = np.frombuffer(self._cmap, dtype=np.uint8)
                return self._cmap_view[start:min(start + length + 16, size)]      # (16 spare bytes where the file has them: the wrapper wants them behind the last chunk and would copy the range to get them)
        except (OSError, ValueError, AttributeError):
            return None

    def _pread_pinned(self, length, start):
        """`length` bytes at `start` of the compressed file as a uint8 view of a page-locked buffer (the codec's: the bytes go to
        the device by DMA from where the file system put them -- no fresh pages to fault in for every read, no staging copy);
        reads of a few MB and more are split over PREAD_THREADS threads.  The caller holds self._pin_lock while the view is in use.
        None when the codec has no such buffers (the caller reads into a bytes object then)."""
        alloc = getattr(self.codec, 'host_buffer_take', None) or getattr(self.codec, 'host_buffer', None)
        if alloc is None or not hasattr(os, 'preadv'):
            return None
        if self._pin is None or self._pin.nbytes < length + 64:
            try:
                new = alloc(max(int((length + 64) * 1.5), 16 << 20))
            except Exception:  # noqa: BLE001
                return None
            if self._pin is not None:
                (getattr(self.codec, 'host_buffer_give', None) or (lambda h: h.free()))(self._pin)
            self._pin = new
        mv = memoryview(self._pin.array)
        fd = self.cdata.fileno()

        def part(a, b):
            while a < b:
                got = os.preadv(fd, [mv[a:b]], start + a)
                if got <= 0:
                    break
                a += got
            return a
        if length >= (4 << 20):
            nt = PREAD_THREADS
            if self._io_pool is None:
                self._io_pool = ThreadPool(nt)
            per = (length + nt - 1) // nt
            ends = self._io_pool.starmap(part, [(k * per, min((k + 1) * per, length)) for k in range(nt) if k * per < length])
            assert all(e == min((k + 1) * per, length) for k, e in enumerate(ends))
        else:
            assert part(0, length) == length
        self._pin.array[length:length + 16] = 0                  # (the kernels may read a few bytes past a stream)
        return self._pin.array[:length + 16]

    def _flags(self):
        return _int_flags(self.cmeta.do_time_diff, self.cmeta.do_spatial_diff, self.chunk_order)

    def _decode(self, triples):
        """Decode chunks [(idx, start, length)] not in the cache with ONE codec call; returns
        {idx: array}.  Error mapping as mtscomp.py:618-628."""
        with self._cache_lock:
            return self._decode_locked(triples)

    def _decode_locked(self, triples):
        todo = [t for t in triples if t[0] not in self._cache]
        result = {}
        if todo:
            rows = [self.chunk_bounds[i + 1] - self.chunk_bounds[i] for (i, _, _) in todo]
            consecutive = all(todo[k][1] + todo[k][2] == todo[k + 1][1] for k in range(len(todo) - 1))
            if consecutive and len(todo) > 1 and getattr(self.codec, 'takes_ranges', False):
                base = todo[0][1]                              # one read for the whole byte range
                buf = self._pread(todo[-1][1] + todo[-1][2] - base, base)
                cbufs = (buf, [t[1] - base for t in todo], [t[2] for t in todo])
            else:
                cbufs = [self._pread(length, start) for (_, start, length) in todo]
            status, arrays = self.codec.decompress(cbufs, rows, self.n_channels, self.dtype, self._flags())
            for (idx, _, _), st, arr in zip(todo, status, arrays):
                if st == hip.CHUNK_BADSIZE:
                    raise AssertionError("Chunk #%d does not have the expected size." % idx)
                if st != hip.CHUNK_OK:
                    raise IOError("Compressed chunk #%d is corrupted." % idx)
                result[idx] = arr
        for idx, _, _ in triples:
            if idx in self._cache:
                self._cache.move_to_end(idx)
                result[idx] = self._cache[idx]
        for idx, arr in result.items():
            self._cache[idx] = arr
            self._cache.move_to_end(idx)
        self._trim_cache()
        return result

    def _trim_cache(self):
        """Back to cache_size entries.  The arrays of one codec call are views of one buffer: entries that would keep a
        buffer several times the size of everything cached from it alive (what is left of a big batch) are replaced by
        copies of themselves; views that still account for most of their buffer stay views (no copy, and neighbours keep
        sharing a base, which lets a slice over several cached chunks be joined without copying)."""
        while len(self._cache) > self.cache_size:
            self._cache.popitem(last=False)
        roots = {}
        for idx, arr in self._cache.items():
            root = arr
            while isinstance(root.base, np.ndarray):
                root = root.base
            if root is not arr:
                entry = roots.setdefault(id(root), [root, 0, []])
                entry[1] += arr.nbytes
                entry[2].append(idx)
        for root, cached_bytes, ids in roots.values():
            if root.nbytes > 2 * cached_bytes:
                for idx in ids:
                    self._cache[idx] = self._cache[idx].copy()

    # -- the decoded-chunk caches in HBM: one per lane of the codec (a HipCodec has a lane per device), chunk k on lane k mod lanes
    def _n_lanes(self):
        return max(1, int(getattr(self.codec, 'n_lanes', 1)))

    def _cache_for(self, lane):
        """The cache id of `lane` (created on first use; every lane gets the capacity the Reader was given)."""
        with self._dev_cache_lock:                             # slices may come from several threads (mtscomp.py:422, :648)
            if self._dev_caches is None:
                self._dev_caches = [None] * self._n_lanes()
            if self._dev_caches[lane] is None:
                if len(self._dev_caches) > 1:
                    self._dev_caches[lane] = self.codec.cache_create(self._dev_cache_bytes, lane)
                else:
                    self._dev_caches[lane] = self.codec.cache_create(self._dev_cache_bytes)
            return self._dev_caches[lane]

    @property
    def _dev_cache(self):
        """Lane 0's cache id, None before its first use."""
        return self._dev_caches[0] if self._dev_caches else None

    @staticmethod
    def _raise_for(status_by_chunk):
        """The reference's errors for the first chunk (in file order) that did not decode (mtscomp.py:618-628)."""
        for k in sorted(status_by_chunk):
            st = status_by_chunk[k]
            if st == hip.CHUNK_BADSIZE:
                raise AssertionError("Chunk #%d does not have the expected size." % k)
            if st != hip.CHUNK_OK:
                raise IOError("Compressed chunk #%d is corrupted." % k)

    def _slice_from_device_cache(self, first, last, i0, i1):
        """Rows [i0, i1) -- inside chunks first..last -- through the codec's decoded-chunk cache in HBM: chunks that are
        not resident are read from the file and decoded in one batch (and stay on the device), and only the requested
        rows come back.  None when the slice should take the host path (no device cache, slice too large for it, or the
        chunks are already in the host LRU of read_chunk)."""
        n = last - first + 1
        if not getattr(self.codec, 'device_cache', False) or self._dev_cache_bytes <= 0 or n > DEVICE_CACHE_MAX_CHUNKS:
            return None
        rows = [self.chunk_bounds[i + 1] - self.chunk_bounds[i] for i in range(first, last + 1)]
        if 2 * sum(rows) * self.n_channels * self.dtype.itemsize > self._dev_cache_bytes:
            return None
        if all(i in self._cache for i in range(first, last + 1)):
            return None
        lanes = self._n_lanes()
        if lanes > 1:
            return self._slice_from_lane_caches(first, last, i0, i1, lanes)
        cache = self._cache_for(0)
        keys = list(range(first, last + 1))
        a, b = i0 - self.chunk_bounds[first], i1 - self.chunk_bounds[first]
        present = [int(p) >= self.n_channels for p in self.codec.cache_query(cache, keys)]      # (entries of leading channels only do not count)
        ahead = self._read_ahead(cache, keys, present)              # chunks behind the slice decoded along with its missing ones
        if ahead:
            keys, present = keys + ahead, present + [False] * len(ahead)
            rows = rows + [self.chunk_bounds[k + 1] - self.chunk_bounds[k] for k in ahead]
            n += len(ahead)
        for attempt in range(2):
            need = [k for k, p in zip(keys, present) if not p]
            offs, lens = [0] * n, [0] * n
            base = self.chunk_offsets[need[0]] if need else 0      # one read from the first to the last missing chunk
            nbytes = self.chunk_offsets[need[-1] + 1] - base if need else 0
            for k in need:
                offs[k - first] = self.chunk_offsets[k] - base
                lens[k - first] = self.chunk_offsets[k + 1] - self.chunk_offsets[k]
            # (the page-locked buffer is the Reader's: held from the read until the codec has taken the bytes, released whatever
            #  either of them raises -- a short read of a truncated file is the reference's AssertionError, not a lock left behind)
            buf = self._map_range(nbytes, base) if need else b''     # (a view of the file's mapping: nothing to lock, nothing read here)
            if buf is not None:
                try:
                    status, out = self.codec.cache_read_rows(cache, keys, buf, offs, lens, rows, self.n_channels,
                                                             self.dtype, self._flags(), a, b)
                    break
                except hip.HipError as e:
                    if e.code != hip.E_MISS or attempt:
                        raise
                    present = [False] * n                          # dropped since the query: send everything
                    continue
            with self._pin_lock:
                buf = self._pread_pinned(nbytes, base) if need else b''
                if buf is None:
                    buf = self._pread(nbytes, base)
                try:
                    status, out = self.codec.cache_read_rows(cache, keys, buf, offs, lens, rows, self.n_channels,
                                                             self.dtype, self._flags(), a, b)
                    break
                except hip.HipError as e:
                    if e.code != hip.E_MISS or attempt:
                        raise
                    present = [False] * n                          # dropped since the query: send everything
        with self._ra_lock:
            for k, st in zip(keys[n - len(ahead):], status[n - len(ahead):]) if ahead else ():
                if st == 0:
                    self._ra_pending[k] = True                     # (a damaged chunk ahead is reported when somebody reads it)
        self._raise_for(dict(zip(keys[:n - len(ahead)], status[:n - len(ahead)])))
        return out

    def _read_ahead(self, cache, keys, present):
        """Chunks right behind a slice that are decoded in the same device call as the slice's missing chunks -- a batch of one
        or two chunks costs the device nearly what a batch of four does (the inflate stages of a small batch are one dependency
        chain each), so a reader that comes to them later (the next window of a sequential reader; sooner or later every chunk,
        for random windows over a recording that fits the cache) finds them decoded.  Adaptive like a file system's read-ahead:
        starts at one chunk, one more (up to READ_AHEAD_MAX) whenever a chunk read ahead is used, one less whenever one leaves
        the list of pending ones unused (the list is half the cache long at most); at none, one chunk is tried every 32nd time.
        Nothing is read ahead when all of a slice's chunks are resident."""
        with self._ra_lock:
            for k, p in zip(keys, present):
                if p and self._ra_pending.pop(k, None):
                    self._ra = min(self._ra + 1, READ_AHEAD_MAX)
            if all(present) or READ_AHEAD_MAX <= 0:
                return []
            self._ra_calls += 1
            ra = self._ra if self._ra > 0 else (1 if self._ra_calls % 32 == 0 else 0)
        chunk_bytes = max(1, (self.chunk_bounds[1] - self.chunk_bounds[0]) * self.n_channels * self.dtype.itemsize)
        cap = max(8, min(self._dev_cache_bytes // chunk_bytes // 2, 1024))
        ra = min(ra, max(0, DEVICE_CACHE_MAX_CHUNKS - len(keys)), int(self._dev_cache_bytes // chunk_bytes // 4))
        cand = list(range(keys[-1] + 1, min(keys[-1] + 1 + ra, self.n_chunks)))
        if not cand:
            return []
        ahead = []
        for k, p in zip(cand, self.codec.cache_query(cache, cand)):
            if int(p) >= self.n_channels:
                break                                              # (one read covers the missing chunks: it ends at the first resident one)
            ahead.append(k)
        with self._ra_lock:
            while self._ra_pending and len(self._ra_pending) + len(ahead) > cap:      # the oldest pending ones have had their chance
                self._ra_pending.pop(next(iter(self._ra_pending)))
                self._ra = max(self._ra - 1, 0)
        return ahead

    def _slice_from_lane_caches(self, first, last, i0, i1, lanes):
        """The same over several lanes: every lane reads, decodes and keeps its own chunks (k mod lanes) and copies the rows of
        [i0, i1) they hold straight into their place in the result, all lanes at once."""
        out = np.empty((i1 - i0, self.n_channels), dtype=self.dtype)
        keys = list(range(first, last + 1))
        status = {}

        def run(g):
            cache = self._cache_for(g)
            for k in keys[(g - first) % lanes::lanes]:
                c0, c1 = self.chunk_bounds[k], self.chunk_bounds[k + 1]
                lo, hi = max(i0, c0), min(i1, c1)
                present = int(self.codec.cache_query(cache, [k])[0]) >= self.n_channels
                for attempt in range(2):
                    length = 0 if present else self.chunk_offsets[k + 1] - self.chunk_offsets[k]
                    buf = self._pread(length, self.chunk_offsets[k]) if length else b''
                    try:
                        st, _ = self.codec.cache_read_rows(cache, [k], buf, [0], [length], [c1 - c0], self.n_channels, self.dtype,
                                                           self._flags(), lo - c0, hi - c0, out=out[lo - i0:hi - i0])
                        break
                    except hip.HipError as e:
                        if e.code != hip.E_MISS or attempt:
                            raise
                        present = False                            # dropped since the query: send the bytes
                status[k] = st[0]
        owners = sorted({k % lanes for k in keys})
        self.codec.run_lanes(lambda j: run(owners[j]), len(owners))
        self._raise_for(status)
        return out

    def _gather_request(self, item):
        """(i0, i1, row_step, c0, c1, col_step, squeeze) when the index is a rectangle the device gather serves, else None."""
        if isinstance(item, slice):
            item = (item, slice(None))
        if not (isinstance(item, tuple) and len(item) == 2 and isinstance(item[0], slice)):
            return None
        rs = 1 if item[0].step is None else item[0].step
        if not isinstance(rs, (int, np.integer)) or rs < 1:
            return None
        cols, squeeze = item[1], False
        if isinstance(cols, (int, np.integer)):
            c = int(cols) + (self.n_channels if cols < 0 else 0)
            if not 0 <= c < self.n_channels:
                return None                                    # (numpy raises IndexError: let it)
            c0, c1, cs, squeeze = c, c + 1, 1, True
        elif isinstance(cols, slice):
            c0, c1, cs = cols.indices(self.n_channels)
            if cs < 1:
                return None
            c1 = max(c0, c1)
        else:
            return None
        i0 = self._validate_index(item[0].start, 0)
        i1 = self._validate_index(item[0].stop, self.n_samples)
        return i0, max(i0, i1), int(rs), c0, c1, cs, squeeze

    def read_slices(self, items, _fallback=True):
        """Several index expressions ``r[rows, columns]`` / ``r[rows]`` in ONE device call per lane: the chunks they touch are
        decoded (or found in the decoded-chunk cache in HBM), the requested rows and columns are gathered on the device and only
        they cross the bus (the reference decodes whole chunks and slices on the host, mtscomp.py:835-842).  Returns the list
        of arrays; items the device gather does not serve go through ``__getitem__`` one by one."""
        reqs = [self._gather_request(it) for it in items]
        usable = getattr(self.codec, 'device_cache', False) and hasattr(self.codec, 'cache_read_slices') and \
            self._dev_cache_bytes > 0 and all(r is not None for r in reqs)
        spans = []
        lanes = self._n_lanes()
        if usable:
            for i0, i1, _, _, _, _, _ in reqs:
                if i1 <= i0:
                    spans.append(None)
                    continue
                first, last = self._chunks_for_interval(i0, i1)
                if last > first and self.chunk_bounds[last] >= i1:
                    last -= 1
                spans.append((first, last))
            keys = sorted({k for sp in spans if sp for k in range(sp[0], sp[1] + 1)})
            rows = [self.chunk_bounds[k + 1] - self.chunk_bounds[k] for k in keys]
            # the limits are PER LANE (chunk k lives on lane k mod lanes: every other chunk with two lanes lands on one of them)
            per_lane = [[r for k, r in zip(keys, rows) if k % lanes == g] for g in range(lanes)]
            usable = len(keys) > 0 and all(len(rs) <= DEVICE_CACHE_MAX_CHUNKS and
                                           2 * sum(rs) * self.n_channels * self.dtype.itemsize <= self._dev_cache_bytes for rs in per_lane)
        if not usable:
            return [self[it] for it in items] if _fallback else None
        # Requests that stay within the leading channels of channel-major chunks need only a prefix of every chunk's stream:
        # the codec inflates a chunk that is not resident just that far, from a prefix of its compressed bytes (the channels
        # compress about equally: the share of the bytes plus a margin; if that falls short the codec says so and the whole
        # chunk is sent).  The reference inflates whole chunks and drops the columns on the host (mtscomp.py:835-842).
        # Only with partial_decode=True: such a read cannot check the chunk's adler32 (the reference always does, mtscomp.py:618-621).
        n_lead = max([r[4] for r in reqs] or [self.n_channels])     # (over ALL requests: the codec checks every one against it)
        leading = self.partial_decode and bool(getattr(self.codec, 'leading_channels', False)) and self.chunk_order == 'F' and \
            self.dtype.kind in 'iu' and 0 < 2 * n_lead <= self.n_channels
        if lanes == 1:
            where = {k: j for j, k in enumerate(keys)}
            cum = np.concatenate(([0], np.cumsum(rows)))
            requests = []
            for (i0, i1, rs, c0, c1, cs, _), sp in zip(reqs, spans):
                a = int(cum[where[sp[0]]]) + i0 - self.chunk_bounds[sp[0]] if sp else 0
                requests.append((a, a + (i1 - i0), rs, c0, c1, cs))
            status, arrays = self._lane_read_slices(self._cache_for(0), keys, requests, n_lead if leading else None)
            self._raise_for(dict(zip(keys, status)))
            return [a[:, 0] if r[6] else a for a, r in zip(arrays, reqs)]
        # several lanes: a request is cut where it crosses from one chunk into the next; every lane gathers the pieces that lie in
        # its chunks (k mod lanes) in one call, all lanes at once; the pieces of a request are joined on the host
        lane_keys = {g: [k for k in keys if k % lanes == g] for g in sorted({k % lanes for k in keys})}
        lane_reqs = {g: [] for g in lane_keys}                      # per lane: (request index, piece index, request tuple)
        n_pieces = []
        for q, ((i0, i1, rs, c0, c1, cs, _), sp) in enumerate(zip(reqs, spans)):
            pieces = 0
            for k in (range(sp[0], sp[1] + 1) if sp else ()):
                b0, b1 = self.chunk_bounds[k], self.chunk_bounds[k + 1]
                lo, hi = max(i0, b0), min(i1, b1)
                start = i0 + -(-(lo - i0) // rs) * rs               # the first row of the request's grid inside the chunk
                if start >= hi:
                    continue
                g = k % lanes
                before = sum(self.chunk_bounds[j + 1] - self.chunk_bounds[j] for j in lane_keys[g] if j < k)      # rows of the lane's chunks in front
                lane_reqs[g].append((q, pieces, (before + start - b0, before + hi - b0, rs, c0, c1, cs)))
                pieces += 1
            n_pieces.append(pieces)
        parts = [[None] * n for n in n_pieces]
        status = {}
        owners = list(lane_keys)

        def run(j):
            g = owners[j]
            st, arrays = self._lane_read_slices(self._cache_for(g), lane_keys[g], [r for _, _, r in lane_reqs[g]], n_lead if leading else None)
            status.update(zip(lane_keys[g], st))
            for (q, piece, _), arr in zip(lane_reqs[g], arrays):
                parts[q][piece] = arr
        self.codec.run_lanes(run, len(owners))
        self._raise_for(status)
        out = []
        for q, r in enumerate(reqs):
            ncol = len(range(r[3], r[4], r[5]))
            arr = parts[q][0] if len(parts[q]) == 1 else np.concatenate(parts[q], axis=0) if parts[q] else np.zeros((0, ncol), dtype=self.dtype)
            out.append(arr[:, 0] if r[6] else arr)
        return out

    def _lane_read_slices(self, cache, keys, requests, n_lead):
        """One cache_read_slices call on one lane's cache: `requests` index the concatenation of the chunks `keys`; the bytes of the
        chunks that are not resident are read first (one read per run of neighbours).  n_lead: the requests stay below that many
        leading channels and a chunk that is not resident is decoded only that far, from a prefix of its bytes; if that falls short
        -- or an entry was dropped between the query and the call -- everything is sent once more, whole.  -> (status, arrays)."""
        where = {k: j for j, k in enumerate(keys)}
        rows = [self.chunk_bounds[k + 1] - self.chunk_bounds[k] for k in keys]
        held = self.codec.cache_query(cache, keys)                  # channels every resident entry holds (0: not resident)
        present = [int(h) >= (n_lead or self.n_channels) for h in held]      # bytes are sent for entries that are too narrow only
        for attempt in range(2):
            leading = bool(n_lead) and attempt == 0
            offs, lens, parts, at = [0] * len(keys), [0] * len(keys), [], 0
            need = [k for k, p in zip(keys, present) if not p]
            j = 0
            while j < len(need):                                # one read per run of neighbouring missing chunks
                e = j
                while not leading and e + 1 < len(need) and need[e + 1] == need[e] + 1:
                    e += 1
                base = self.chunk_offsets[need[j]]
                nbytes = self.chunk_offsets[need[e] + 1] - base
                if leading:                                     # (one chunk: a prefix of its bytes)
                    nbytes = min(nbytes, int(nbytes * n_lead / self.n_channels * 1.3) + 32768)
                parts.append(self._pread(nbytes, base))
                for k in need[j:e + 1]:
                    offs[where[k]] = at + self.chunk_offsets[k] - base
                    lens[where[k]] = min(self.chunk_offsets[k + 1] - self.chunk_offsets[k], nbytes)
                at += len(parts[-1])
                j = e + 1
            try:
                # the second attempt is a plain whole-chunk decode (every check runs: a chunk the prefix decoder cannot follow, or
                # one damaged inside the prefix, gets the reference's verdict instead of a miss)
                extra = {'n_leading': n_lead} if leading else {}
                return self.codec.cache_read_slices(cache, keys, b''.join(parts), offs, lens, rows,
                                                    self.n_channels, self.dtype, self._flags(), requests, **extra)
            except hip.HipError as e:
                if e.code != hip.E_MISS or attempt:
                    raise
                present = [False] * len(keys)                  # dropped since the query (or a prefix fell short): send everything

    # -- per-window statistics on the device (an extension: the reference's users reduce Reader[...] with numpy)
    def _stats_channels(self, channels):
        """(column indices as an int array, squeeze) for an int, a slice with step >= 1 or a 1-D sequence of ints."""
        nc = self.n_channels
        if isinstance(channels, (int, np.integer)):
            c = int(channels)
            if not -nc <= c < nc:
                raise IndexError("channel %d is out of bounds for %d channels" % (c, nc))
            return np.array([c % nc], dtype=np.int64), True
        if isinstance(channels, slice):
            c0, c1, cs = channels.indices(nc)
            if cs < 1:
                raise ValueError("window_stats: a channel slice needs a step >= 1")
            return np.arange(c0, c1, cs, dtype=np.int64), False
        cols = np.asarray(channels)
        if cols.ndim != 1 or (cols.size and cols.dtype.kind not in 'iu'):
            raise IndexError("window_stats: channels must be an int, a slice or a 1-D sequence of ints")
        cols = cols.astype(np.int64)
        if cols.size and (cols.min() < -nc or cols.max() >= nc):
            raise IndexError("channel index out of bounds for %d channels" % nc)
        return cols % nc if cols.size else cols, False

    def window_stats(self, window, start=0, stop=None, channels=slice(None)):
        """Per-window, per-channel statistics of rows [start, stop) computed on the device: only the results cross the bus.
        Windows are [start + w * window, min(start + (w + 1) * window, stop)); window=None is one window over the range.
        start / stop follow Reader[...] (None, negative, clipped).  channels: an int (the arrays are then 1-D), a slice with
        step >= 1, or a sequence of ints.  Returns a Bunch: count (n_windows,) int64; min, max in the recording's dtype (NaN
        propagates like np.min / np.max); sum (int64 with numpy's wrap for integers, float64 for floats); sumsq (float64; exact
        for 1/2-byte integers); mean = sum / count and rms = sqrt(sumsq / count) in float64; start, stop, window, channels.
        Chunks resident in the device cache are read where they lie; the others are decoded in a transient workspace and NOT
        kept.  A damaged chunk raises the IOError of Reader[...]."""
        self._need_codec('window_stats', 'window_stats', 'reduces')
        i0, i1 = self._row_range(start, stop)
        window = _window_rows(window, i0, i1)
        cols, squeeze = self._stats_channels(channels)
        n_win = -(-(i1 - i0) // window)
        t_dt, s_dt, q_dt = hip.stats_dtypes(self.dtype)
        shape = (n_win, cols.size)
        fi = np.finfo if self.dtype.kind == 'f' else np.iinfo
        mn = np.full(shape, np.inf if self.dtype.kind == 'f' else fi(self.dtype).max, dtype=t_dt)
        mx = np.full(shape, -np.inf if self.dtype.kind == 'f' else fi(self.dtype).min, dtype=t_dt)
        sm, sq, cnt = np.zeros(shape, s_dt), np.zeros(shape, q_dt), np.zeros(n_win, np.int64)
        # calls: runs of chunks whose compressed bytes and partial results (32 bytes per column and tile) fit one device call
        tile_rows = min(window, 512)
        calls = self._chunk_runs(self._chunks_in(i0, i1) if n_win and cols.size else [], WINDOW_STATS_CALL_BYTES, WINDOW_STATS_SLAB_BYTES,
                                 lambda k: (-(-(self.chunk_bounds[k + 1] - self.chunk_bounds[k]) // tile_rows) + 1) * cols.size * 32)
        status = {}
        for run in calls:
            lo, hi = max(i0, self.chunk_bounds[run[0]]), min(i1, self.chunk_bounds[run[-1] + 1])
            w0, w1 = (lo - i0) // window, -(-(hi - i0) // window)
            rb, re = i0 + w0 * window, min(i1, i0 + w1 * window)
            sl = slice(w0, w1)
            for res in self._on_owner_lanes(self.codec.window_stats, run, status, rb, re, window, cols):      # lanes in order: the float sums are the same every time
                mn[sl] = np.minimum(mn[sl], res['min'])
                mx[sl] = np.maximum(mx[sl], res['max'])
                sm[sl] += res['sum']
                sq[sl] += res['sumsq']
                cnt[sl] += res['count']
        self._raise_for(status)
        if not cols.size:                                           # (no columns: nothing to read, the rows are counted here)
            cnt[:] = np.minimum(window, i1 - i0 - window * np.arange(n_win))
        sumsq = sq.astype(np.float64)                               # (the exact sums of squares: converted once, here)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = sm.astype(np.float64) / cnt[:, None]
            rms = np.sqrt(sumsq / cnt[:, None])
        out = Bunch(count=cnt, min=mn, max=mx, sum=sm, sumsq=sumsq, mean=mean, rms=rms, start=i0, stop=i1, window=window, channels=cols)
        if squeeze:
            for key in ('min', 'max', 'sum', 'sumsq', 'mean', 'rms'):
                out[key] = out[key][:, 0]
        return out

    # -- what the device reductions share: argument checks, the cut of a range into device calls, the lanes of a call
    def _need_codec(self, what, method, does):
        if not callable(getattr(self.codec, method, None)):
            raise NotImplementedError("%s needs a codec that %s on the device (HipCodec); %r has none"
                                      % (what, does, getattr(self.codec, 'name', self.codec)))

    def _row_range(self, start, stop):
        """Rows [i0, i1) for start / stop as Reader[...] takes them (None, negative, clipped)."""
        i0 = self._validate_index(start, 0)
        return i0, max(i0, self._validate_index(stop, self.n_samples))

    def _lane_cache(self, lane):
        """The cache a reduction on `lane` reads resident chunks from, 0 when the Reader keeps none."""
        return self._cache_for(lane) if getattr(self.codec, 'device_cache', False) and self._dev_cache_bytes > 0 else 0

    def _chunks_in(self, lo, hi):
        """The chunks that hold rows of [lo, hi), in order."""
        first = bisect.bisect_right(self.chunk_bounds, lo) - 1
        last = bisect.bisect_left(self.chunk_bounds, hi) - 1
        return [k for k in range(max(first, 0), min(last, self.n_chunks - 1) + 1)
                if self.chunk_bounds[k + 1] > max(lo, self.chunk_bounds[k]) and self.chunk_bounds[k] < hi]

    def _chunk_runs(self, chunks, max_bytes, max_weight=None, weight=None):
        """The tile family's calls (window_stats, rank_hist): `chunks` cut into runs of at most max_bytes compressed bytes and, given
        weight(k), at most max_weight in all; a run holds one chunk at least."""
        runs, run, nbytes, total = [], [], 0, 0
        for k in chunks:
            b = self.chunk_offsets[k + 1] - self.chunk_offsets[k]
            t = weight(k) if weight else 0
            if run and (nbytes + b > max_bytes or (weight and total + t > max_weight)):
                runs.append(run)
                run, nbytes, total = [], 0, 0
            run.append(k)
            nbytes, total = nbytes + b, total + t
        if run:
            runs.append(run)
        return runs

    def _on_owner_lanes(self, fn, run, status, *args):
        """One call of the tile family: the chunks of `run` on their owner lanes (chunk k on lane k mod lanes: where the cache holds it),
        all lanes at once.  Every chunk is in one lane's call: its status goes into `status`.  -> the lanes' results, in lane order."""
        lanes = self._n_lanes()
        owners = sorted({k % lanes for k in run})
        parts = [None] * len(owners)

        def one(j):
            g = owners[j]
            keys = [k for k in run if k % lanes == g]
            st, res = self._lane_call(fn, self._lane_cache(g), keys, g, *args)
            parts[j] = (keys, st, res)
        self.codec.run_lanes(one, len(owners))
        for keys, st, _ in parts:
            status.update(zip(keys, st))
        return [res for _, _, res in parts]

    def _halo_cuts(self, lo, hi, max_bytes, u0, u1, unit_at):
        """The calls of decimate and detect: units [u0, u1) (outputs, rows) cut where the compressed bytes of the chunks of rows [lo, hi)
        pass max_bytes; unit_at(row): the first unit that starts at or after a chunk boundary.  -> the cut list, u0 first, u1 last."""
        first = bisect.bisect_right(self.chunk_bounds, lo) - 1
        last = bisect.bisect_right(self.chunk_bounds, hi - 1) - 1
        cuts, acc = [u0], 0
        for k in range(first, last + 1):
            b = self.chunk_offsets[k + 1] - self.chunk_offsets[k]
            if acc and acc + b > max_bytes:
                u = unit_at(self.chunk_bounds[k])
                if u > cuts[-1]:
                    cuts.append(u)
                    acc = 0
            acc += b
        cuts.append(u1)
        return cuts

    def _chunk_span(self, lo, hi):
        """The adjacent chunks that hold rows [lo, hi), lo < hi, as a list of keys."""
        return list(range(bisect.bisect_right(self.chunk_bounds, lo) - 1, bisect.bisect_right(self.chunk_bounds, hi - 1)))

    def _budget_cuts(self, lo, hi, max_bytes, i0, i1, row_bytes, out_bytes):
        """The calls of project, correlate and residual: rows [i0, i1) cut at the chunk boundaries where the compressed bytes of the
        chunks of the rows [lo, hi) they read pass max_bytes, and again so that a call's result (row_bytes a row) stays within
        out_bytes.  -> the cut list, i0 first, i1 last."""
        rows = max(1, out_bytes // row_bytes)
        base = self._halo_cuts(lo, hi, max_bytes, i0, i1, lambda row: min(i1, max(i0, row)))
        return [u for a, b in zip(base[:-1], base[1:]) for u in range(a, b, rows)] + [i1]

    def _support(self, a, b, R, before, after, n_taps):
        """The file rows [lo, hi) that the results of rows [a, b) read: the rows themselves and R either side (an exclusion), from
        `before` rows before to after - 1 rows after each of those (a template; 0 and 1: the row alone), and the filter's support of
        all of them, inside the recording."""
        half = (n_taps - 1) // 2
        return max(0, a - R - before + half - (n_taps - 1)), min(self.n_samples, b + R + after - 1 + half)

    def _filter_args(self, taps, reference, channels, then=None):
        """The arguments that detect, waveforms, correlate, match_templates and residual filter by -> (taps as float64, default [1.0];
        the columns; reference as the library's code; then(cols)).  `then` holds the checks that an op makes of its own arguments
        against the columns: they come before the median's column limit, as they always did."""
        if reference not in (None, 'median'):
            raise ValueError("reference must be None or 'median', got %r" % (reference,))
        taps = _fir_taps([1.0] if taps is None else taps)
        cols, _ = self._stats_channels(channels)
        more = then(cols) if then else None
        if reference and cols.size > hip.DETECT_MAX_REF_COLS:
            raise ValueError("a median reference takes at most %d columns, got %d" % (hip.DETECT_MAX_REF_COLS, cols.size))
        return taps, cols, 1 if reference else 0, more

    def _halo_parts(self, fn, cuts, part, again=None):
        """The halo family's calls (decimate, detect, welch, gram): every [cuts[i], cuts[i + 1]) of the op's unit axis (outputs, rows,
        groups) is one round of calls, split into contiguous parts [a, b), one per lane (a part's halo is decoded by that part alone).
        part(a, b) -> (keys, args): the adjacent chunks the part reads and the op's own arguments, or None when it reads nothing.
        again(result, args) -> the arguments of a second call of the part, or None.  A chunk may be in several parts' calls: a
        status that is not CHUNK_OK wins.  Yields (a, b, result without the status) in order; the error of a chunk that did not
        decode is raised after the last."""
        lanes = self._n_lanes()
        status = {}
        for ca, cb in zip(cuts[:-1], cuts[1:]):
            if cb <= ca:
                continue
            nl = max(1, min(lanes, cb - ca))
            at = [ca + (cb - ca) * g // nl for g in range(nl + 1)]
            res = [None] * nl

            def one(g, at=at, res=res):
                what = part(at[g], at[g + 1])
                if what is None:
                    return
                keys, args = what
                cache = self._lane_cache(g)
                got = self._lane_call(fn, cache, keys, g, *args)
                more = again(got, args) if again else None
                if more is not None:
                    got = self._lane_call(fn, cache, keys, g, *more)
                res[g] = (keys, got)
            self.codec.run_lanes(one, nl)
            for g in range(nl):
                if res[g] is None:
                    continue
                keys, got = res[g]
                for k, v in zip(keys, got[0]):
                    if v != hip.CHUNK_OK or k not in status:
                        status[k] = v
                yield at[g], at[g + 1], got[1:]
        self._raise_for(status)

    def _lane_call(self, fn, cache, keys, lane, *args):
        """One call of a codec's reduction `fn` (window_stats, rank_hist, decimate, detect, welch or gram) for the chunks `keys` of one lane:
        chunks resident in its cache go without bytes, the others' compressed bytes come from a mapping of the file (or one read); sent
        whole once more if an entry was dropped between the query and the call.  -> what `fn` returns."""
        row0 = [self.chunk_bounds[k] for k in keys]
        rows = [self.chunk_bounds[k + 1] - self.chunk_bounds[k] for k in keys]
        present = [int(p) >= self.n_channels for p in self.codec.cache_query(cache, keys)] if cache else [False] * len(keys)
        for attempt in range(2):
            need = [k for k, p in zip(keys, present) if not p]
            base = self.chunk_offsets[need[0]] if need else 0
            nbytes = self.chunk_offsets[need[-1] + 1] - base if need else 0
            offs = [self.chunk_offsets[k] - base if not p else 0 for k, p in zip(keys, present)]
            lens = [self.chunk_offsets[k + 1] - self.chunk_offsets[k] if not p else 0 for k, p in zip(keys, present)]
            buf = self._map_range(nbytes, base) if need else b''
            if buf is None:
                buf = self._pread(nbytes, base)
            try:
                return fn(cache, keys, row0, buf, offs, lens, rows, self.n_channels, self.dtype, self._flags(), *args, lane=lane)
            except hip.HipError as e:
                if e.code != hip.E_MISS or attempt:
                    raise
                present = [False] * len(keys)                       # dropped since the query: send everything

    # -- exact order statistics on the device (an extension: the reference's users sort Reader[...] on the host)
    def _rank_setup(self, what, start, stop, window, channels, filtered=False):
        self._need_codec(what, 'filtered_rank_hist' if filtered else 'rank_hist', 'selects in the filtered rows' if filtered else 'selects')
        i0, i1 = self._row_range(start, stop)
        window = _window_rows(window, i0, i1)
        if min(window, i1 - i0) >= 1 << 32:
            raise ValueError("windows of 2^32 rows or more are not supported")
        cols, squeeze = self._stats_channels(channels)
        n_win = -(-(i1 - i0) // window)
        count = np.minimum(window, i1 - i0 - window * np.arange(n_win, dtype=np.int64)).astype(np.int64)
        return i0, i1, window, cols, squeeze, count

    def _rank_center(self, center, n_win, n_cols):
        c = np.asarray(0.0 if center is None else center)
        if c.dtype.kind not in 'fiub':
            raise ValueError("center must be None or an array of numbers")
        try:
            return np.ascontiguousarray(np.broadcast_to(c.astype(np.float64), (n_win, n_cols)))
        except ValueError:
            raise ValueError("center of shape %r does not broadcast to (n_windows, n_channels) = %r" % (c.shape, (n_win, n_cols))) from None

    def _rank_scan(self, i0, i1, window, cols, ranks, mode=0, center=None, filt=None):
        """The order statistics `ranks` (n_windows, R) int64, 0 <= rank < rows of the window, of every (window, column) cell of the
        grid: a most-significant-digit radix select whose rounds are mts_rank_hist calls.  filt = (taps, reference code): the items
        are the float32 filtered rows z of detect instead of the decoded ones, and the rounds mts_filtered_rank_hist calls.  -> (keys (n_windows, R, C) uint64 --
        hip.rank_values turns them into items --, has_nan (n_windows, C), rounds: the mts_rank_hist passes made).  The windows are scanned in runs whose histograms fit
        QUANTILE_SLAB_BYTES, RANK_SELECTORS ranks at a time; a run is at most ceil(key_bits / 8) rounds, each one pass over its
        chunks."""
        n_win, R = ranks.shape
        S, nb = hip.RANK_SELECTORS, 1 << hip.RANK_BITS
        out = np.zeros((n_win, R, cols.size), np.uint64)
        has_nan = np.zeros((n_win, cols.size), bool)
        rounds = 0
        if not n_win or not cols.size or not R:
            return out, has_nan, rounds
        dtype = np.dtype(np.float32) if filt else self.dtype       # the items' type: what the keys are made of
        nan_key = hip.rank_key_nan(dtype, mode)
        floats = bool(mode) or dtype.kind == 'f'
        per_win = S * (4 * nb + 16) * cols.size
        run_wins = max(1, QUANTILE_SLAB_BYTES // per_win)
        status = {}
        for ws in range(0, n_win, run_wins):
            we = min(n_win, ws + run_wins)
            rb, re = i0 + ws * window, min(i1, i0 + we * window)
            if filt:                                                # (the cut list of the run's rows: every [cuts[i], cuts[i + 1]) a round of calls)
                calls = self._halo_cuts(rb, re, QUANTILE_CALL_BYTES, rb, re, lambda row: row)
            else:
                calls = self._chunk_runs(self._chunks_in(rb, re), QUANTILE_CALL_BYTES)
            cen = center[ws:we] if mode else None
            for r0 in range(0, R, S):
                rk = ranks[ws:we, r0:r0 + S]
                got = rk.shape[1]
                if got < S:                                         # (an odd rank out: the second selector repeats it and shares its histogram)
                    rk = np.concatenate([rk] + [rk[:, -1:]] * (S - got), axis=1)
                keys, kmax0, n_rounds = self._rank_rounds(calls, rb, re, window, cols, mode, cen, rk, status, dtype, filt)
                rounds += n_rounds
                out[ws:we, r0:r0 + got] = keys[:, :got]
                if r0 == 0 and floats:
                    has_nan[ws:we] = kmax0 == nan_key
        return out, has_nan, rounds

    def _rank_rounds(self, calls, rb, re, window, cols, mode, center, ranks, status, dtype, filt=None):
        """The rounds of one run of windows [rb, re) for RANK_SELECTORS ranks per cell.  State per (window, selector, column): the
        candidates are the items with key >> (shift + 8) == pref, the rank `rel` counts among them.  A round's histogram picks the
        digit; the candidates' kmin / kmax (known one round late) tell down to which bit they all agree (bit_length(kmin ^ kmax)): the next digit
        starts there, and kmin == kmax ends the scan.  The
        two ranks of a cell share ONE selector while their candidates are the same set, so that the candidate sets of a cell's
        selectors are always disjoint.  -> (keys (n_windows, S, C) uint64, kmax of the first, prefix-free round (n_windows, C), the rounds made)."""
        S, B = hip.RANK_SELECTORS, hip.RANK_BITS
        nw, C = ranks.shape[0], cols.size
        kb = hip.rank_key_bits(dtype, mode)
        u64 = np.uint64
        rel = np.repeat(ranks[:, :, None].astype(np.int64), C, axis=2)
        shift = np.full((nw, S, C), kb - B, u64)
        pref = np.zeros((nw, S, C), u64)
        ubits = np.full((nw, S, C), B, u64)          # < 8 on a last round whose digit still holds known bits: only digits that agree with `kdig` there count
        kdig = np.zeros((nw, S, C), u64)
        done = np.zeros((nw, S, C), bool)
        val = np.zeros((nw, S, C), u64)
        kmax0 = None
        max_rounds = -(-kb // B)
        digits = np.arange(1 << B, dtype=u64)[None, :, None]
        rnd = 0
        while not done.all():
            assert rnd < max_rounds, 'radix select: more than %d rounds' % max_rounds
            share = ~done[:, 0] & ~done[:, 1] & (pref[:, 0] == pref[:, 1]) & (shift[:, 0] == shift[:, 1])
            sel_shift = np.where(done, -1, shift.astype(np.int64)).astype(np.int32)
            sel_shift[:, 1][share] = -1
            hist, kmin, kmax = self._rank_call(calls, rb, re, window, cols, mode, center, pref, sel_shift, status, filt)
            if rnd == 0:
                kmax0 = kmax[:, 0].copy()
            for s in range(S):
                if s and not share.any():
                    h, kmn, kmx = hist[:, s], kmin[:, s], kmax[:, s]
                elif s and not share.all():
                    h = np.where(share[:, None, :], hist[:, 0], hist[:, s])
                    kmn, kmx = np.where(share, kmin[:, 0], kmin[:, s]), np.where(share, kmax[:, 0], kmax[:, s])
                else:                                               # (selector 1 shares selector 0's candidates)
                    h, kmn, kmx = hist[:, 0], kmin[:, 0], kmax[:, 0]
                act = ~done[:, s]
                if (ubits[:, s] < B).any():                         # (a last round whose digit still holds known bits)
                    ub = ubits[:, s][:, None, :]
                    h = np.where((digits >> ub) == (kdig[:, s][:, None, :] >> ub), h, 0)
                cum = np.cumsum(h, axis=1, dtype=np.int64)
                r = rel[:, s]
                if not (r[act] < cum[:, -1][act]).all():
                    raise RuntimeError("radix select: a rank beyond the rows counted (rows were not counted)")
                dig = np.minimum((cum <= r[:, None, :]).sum(axis=1), (1 << B) - 1)
                below = np.take_along_axis(cum, dig[:, None, :], axis=1)[:, 0] - np.take_along_axis(h, dig[:, None, :], axis=1)[:, 0]
                sh = shift[:, s]
                known = ((pref[:, s] << u64(B)) | dig.astype(u64)) << sh         # every bit from `sh` up
                d = hip.rank_bit_length(kmn ^ kmx)                                         # the candidates of this round agree above bit d
                u = np.minimum(sh, d)
                low = (u64(1) << sh) - u64(1)
                known |= kmn & low & ~((u64(1) << u) - u64(1))
                fin = act & (u == 0)
                val[:, s] = np.where(fin, known, val[:, s])
                go = act & ~fin
                nsh = np.where(u >= B, u - u64(B), u64(0)).astype(u64)
                shift[:, s] = np.where(go, nsh, sh)
                pref[:, s] = np.where(go, known >> (nsh + u64(B)), pref[:, s])
                ubits[:, s] = np.where(go, np.minimum(u, u64(B)), ubits[:, s])
                kdig[:, s] = np.where(go & (u < B), known & u64((1 << B) - 1), u64(0))
                rel[:, s] = np.where(go, r - below, r)
                done[:, s] |= fin
            rnd += 1
        return val, kmax0, rnd

    def _rank_call(self, calls, rb, re, window, cols, mode, center, pref, sel_shift, status, filt=None):
        """One round, the integer partials of its calls added (the order does not matter).  A chunk that did not decode raises the
        error of Reader[...].  The feed -- unfiltered: `calls` are lists of chunk indices (the tile family), every call's chunks on
        their owner lanes.  filt = (taps, reference code): `calls` is the cut list of the rows [rb, re) (the halo family), every part
        (a, b) one mts_filtered_rank_hist call that counts its rows on the grid of the windows it meets, with the adjacent chunks
        of its filter support."""
        S, nb = hip.RANK_SELECTORS, 1 << hip.RANK_BITS
        nw, C = pref.shape[0], cols.size
        hist = np.zeros((nw, S, nb, C), np.uint32)
        kmin = np.full((nw, S, C), hip.RANK_KEY_NONE, np.uint64)
        kmax = np.zeros((nw, S, C), np.uint64)

        def grid(lo, hi):
            """The windows that hold the rows [lo, hi): (their slice, the grid's rows, its center and selectors)."""
            w0, w1 = (lo - rb) // window, -(-(hi - rb) // window)
            sl = slice(w0, w1)
            cen = None if center is None else np.ascontiguousarray(center[sl])
            return sl, (rb + w0 * window, min(re, rb + w1 * window)), (mode, cen, np.ascontiguousarray(pref[sl]), np.ascontiguousarray(sel_shift[sl]))

        def unfiltered():
            for run in calls:
                sl, (cb, ce), sel = grid(max(rb, self.chunk_bounds[run[0]]), min(re, self.chunk_bounds[run[-1] + 1]))
                for res in self._on_owner_lanes(self.codec.rank_hist, run, status, cb, ce, window, cols, *sel):
                    yield sl, res

        def filtered():
            taps, ref_code = filt

            def part(a, b):
                _, (cb, ce), sel = grid(a, b)
                keys = self._chunk_span(*self._support(a, b, 0, 0, 1, int(taps.size)))
                return keys, (0, self.n_samples, taps, cols, ref_code, cb, ce, window, a, b) + sel
            for a, b, (res,) in self._halo_parts(self.codec.filtered_rank_hist, calls, part):
                yield grid(a, b)[0], res

        for sl, res in (filtered() if filt else unfiltered()):
            hist[sl] += res['hist']
            kmin[sl] = np.minimum(kmin[sl], res['kmin'])
            kmax[sl] = np.maximum(kmax[sl], res['kmax'])
        self._raise_for(status)
        return hist, kmin, kmax

    def _rank_filter(self, taps, reference, channels):
        """taps= / reference= of quantile, median and mad -> None when neither is given (the decoded items are ordered), else (taps as
        float64, reference as the library's code), checked as detect checks them."""
        if taps is None and reference is None:
            return None
        taps, _, ref_code, _ = self._filter_args(taps, reference, channels)
        return taps, ref_code

    def quantile(self, q, start=0, stop=None, channels=slice(None), window=None, method='linear', center=None, absolute=False, taps=None,
                 reference=None):
        """Exact per-window, per-channel quantiles of rows [start, stop), selected on the device: only digit histograms cross the
        bus.  start / stop / window / channels as window_stats (window=None: one window over the range).  q: a float or a 1-D
        sequence of floats in [0, 1].  For a window of n rows the position v = q * (n - 1) is computed exactly (as a fraction), index
        = floor(v), frac = v - index; the device delivers the order statistics lower = sort(x)[index] and upper = sort(x)[min(index + 1,
        n - 1)], and the result is formed in float64 from lo = float64(lower), hi = float64(upper) -- 'linear': lo + (hi - lo) * frac;
        'lower': lo; 'higher': hi if frac > 0 else lo; 'midpoint': (lo + hi) / 2 if frac > 0 else lo; 'nearest': lo below a half, hi
        above, the even index at exactly a half (numpy's rule).
        center / absolute change what is ordered: float64(x) - c[w, j], or its absolute value; c broadcasts to (n_windows, n_channels),
        None is 0.  lower / upper are then float64, otherwise they are in the recording's dtype.
        Ordering: as np.sort; every NaN, of either sign, sorts last; -0.0 and +0.0 are one key and come back as +0.0 (compare by
        value); a window that holds a NaN gives a NaN quantile, as np.quantile does, while lower / upper still hold the order
        statistics; integers are ordered in their own type, 8-byte ones exactly.
        Returns a Bunch: count (n_windows,); q (n_q,); quantile (n_windows, n_q, C) float64; lower, upper of that shape; index
        (n_windows, n_q) int64 and frac float64; start, stop, window, channels, method; rounds, the passes over the chunks the call made
        (mts_rank_hist rounds: what a cold scan decodes).  A scalar q drops the n_q axis, an int channel
        the C axis.  Chunks resident in the device cache are read where they lie; the others are decoded in a transient workspace
        and NOT kept.  Every window costs a histogram however few rows it has: small windows are correct, not fast.  A damaged chunk
        raises the IOError of Reader[...].
        taps= / reference= (as detect takes them; either given): what is ordered is z[t, j], the filtered rows of detect -- float32,
        the bytes of decimate(1, taps=taps, edge='recording', dtype=float32) on `channels` (taps=None is [1.0]) minus, with
        reference='median', the float32 median over the selected columns of each row; the bytes of residual([], ...).  z is made
        and counted on the device slab by slab and never crosses the bus.  The items are float32: lower / upper are float32 without
        center / absolute, everything else is the contract above for a float32 recording (a NaN in a row makes, with the median
        reference, every column's window NaN).  The Bunch then also carries taps (the float64 array used) and reference; rounds
        counts mts_filtered_rank_hist rounds.  The same bits whatever the lanes, calls, pieces, slabs or cache residency; a damaged
        chunk in the filter's support raises the IOError of Reader[...]."""
        if method not in QUANTILE_METHODS:
            raise ValueError("method must be one of %r, got %r" % (QUANTILE_METHODS, method))
        try:
            qa = np.asarray(q, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("q must be a float or a 1-D sequence of floats in [0, 1]") from None
        q_scalar = qa.ndim == 0
        qa = qa.reshape(-1) if qa.ndim <= 1 else qa
        if qa.ndim != 1 or np.asarray(q).dtype.kind not in 'fiu' or not ((qa >= 0) & (qa <= 1)).all():
            raise ValueError("q must be a float or a 1-D sequence of floats in [0, 1], got %r" % (q,))
        filt = self._rank_filter(taps, reference, channels)
        i0, i1, window, cols, squeeze, count = self._rank_setup('quantile', start, stop, window, channels, filt is not None)
        n_win, nq = count.size, qa.size
        mode = 2 if absolute else 1 if center is not None else 0
        cen = self._rank_center(center, n_win, cols.size) if mode else None
        index = np.zeros((n_win, nq), np.int64)
        frac = np.zeros((n_win, nq), np.float64)
        lengths = sorted(set(count.tolist()))                      # (two values at most: the window and the rest)
        uniq = {}
        for n in lengths:
            rows = count == n
            for k, qv in enumerate(qa.tolist()):
                v = Fraction(qv) * (n - 1)
                j = v.numerator // v.denominator
                index[rows, k], frac[rows, k] = j, float(v - j)
            w = int(np.argmax(rows))
            uniq[n] = np.unique(np.concatenate((index[w], np.minimum(index[w] + 1, n - 1))))      # the distinct ranks of such a window
        upper_i = np.minimum(index + 1, count[:, None] - 1)
        R = max((u.size for u in uniq.values()), default=0)
        rk = np.zeros((n_win, R), np.int64)
        pos_lo, pos_hi = np.zeros((n_win, nq), np.int64), np.zeros((n_win, nq), np.int64)
        for n in lengths:                                           # (windows of one length share their ranks; padded with the last)
            rows, u = count == n, uniq[n]
            w = int(np.argmax(rows))
            rk[rows] = np.concatenate((u, np.repeat(u[-1:], R - u.size)))
            pos_lo[rows], pos_hi[rows] = np.searchsorted(u, index[w]), np.searchsorted(u, upper_i[w])
        keys, has_nan, rounds = self._rank_scan(i0, i1, window, cols, rk, mode, cen, filt)
        vals = hip.rank_values(keys, np.float32 if filt else self.dtype, mode)      # (n_win, R, C)
        if n_win:
            lower, upper = np.take_along_axis(vals, pos_lo[:, :, None], axis=1), np.take_along_axis(vals, pos_hi[:, :, None], axis=1)
        else:
            lower = upper = np.zeros((0, nq, cols.size), vals.dtype)
        lo, hi, g = lower.astype(np.float64), upper.astype(np.float64), frac[:, :, None]
        with np.errstate(invalid='ignore', over='ignore'):
            if method == 'linear':
                res = lo + (hi - lo) * g
            elif method == 'lower':
                res = lo.copy()
            elif method == 'higher':
                res = np.where(g > 0, hi, lo)
            elif method == 'midpoint':
                res = np.where(g > 0, (lo + hi) / 2, lo)
            else:
                even = (index % 2 == 0)[:, :, None]
                res = np.where(g < 0.5, lo, np.where(g > 0.5, hi, np.where(even, lo, hi)))
        res = np.where(has_nan[:, None, :], np.nan, res)
        out = Bunch(count=count, q=qa, quantile=res, lower=lower, upper=upper, index=index, frac=frac, start=i0, stop=i1, window=window,
                    channels=cols, method=method, rounds=rounds)
        if filt:
            out.taps, out.reference = filt[0], reference
        if squeeze:
            for key in ('quantile', 'lower', 'upper'):
                out[key] = out[key][:, :, 0]
        if q_scalar:
            for key in ('quantile', 'lower', 'upper', 'index', 'frac'):
                out[key] = out[key][:, 0]
        return out

    def median(self, start=0, stop=None, channels=slice(None), window=None, taps=None, reference=None):
        """Per-window, per-channel median of rows [start, stop) as float64, (n_windows, C) (an int channel drops C): quantile(0.5)
        with method='midpoint' -- (float64(lower) + float64(upper)) / 2 over the two middle order statistics of a window of an even
        number of rows, the middle one of an odd number --, the value of np.median(r[w0:w1, channels].astype(np.float64), axis=0),
        NaN for a window that holds one.  Ordering rules, cache use and errors as quantile.  taps= / reference= as quantile: the
        median of the filtered rows z, np.median(z.astype(np.float64), axis=0)."""
        return self.quantile(0.5, start, stop, channels=channels, window=window, method='midpoint', taps=taps, reference=reference).quantile

    def mad(self, start=0, stop=None, channels=slice(None), window=None, center='median', taps=None, reference=None):
        """Per-window, per-channel median absolute deviation median(|float64(x) - center|) of rows [start, stop): two scans on the
        device, the median, then the median of the absolute deviations from it.  center: 'median', or an array that broadcasts to
        (n_windows, C) (zeros: the spike-band noise estimate median(|x|); divide by 0.6745 for a standard deviation).  Returns a
        Bunch: count, center, mad (n_windows, C) float64 (an int channel drops C), start, stop, window, channels, rounds (the passes
        over the chunks of both scans).  Per window it
        equals scipy.stats.median_abs_deviation(x.astype(np.float64), axis=0), NaN for a window that holds one.  Ordering rules,
        cache use and errors as quantile.  taps= / reference= as quantile: x is the filtered rows z, and the Bunch also carries taps and
        reference -- mad(center=0.0, taps=highpass_taps(300, sample_rate), reference='median').mad / 0.6745 is the spike-band noise
        level that detect's thresholds are set from."""
        filt = self._rank_filter(taps, reference, channels)
        i0, i1, window, cols, squeeze, count = self._rank_setup('mad', start, stop, window, channels, filt is not None)
        taps = None if filt is None else filt[0]
        if isinstance(center, str):
            if center != 'median':
                raise ValueError("center must be 'median' or an array, got %r" % (center,))
            med = self.quantile(0.5, i0, i1, channels=cols, window=window, method='midpoint', taps=taps, reference=reference)
            cen, rounds = med.quantile.reshape(count.size, cols.size), med.rounds
        else:
            cen, rounds = self._rank_center(center, count.size, cols.size), 0
        res = self.quantile(0.5, i0, i1, channels=cols, window=window, method='midpoint', center=cen, absolute=True, taps=taps, reference=reference)
        dev = res.quantile
        out = Bunch(count=count, center=cen, mad=dev, start=i0, stop=i1, window=window, channels=cols, rounds=rounds + res.rounds)
        if filt:
            out.taps, out.reference = taps, reference
        if squeeze:
            out.center, out.mad = cen[:, 0], dev[:, 0]
        return out

    # -- FIR low-pass + decimation on the device (an extension: the reference's users filter Reader[...] on the host)
    def decimate(self, q, start=0, stop=None, channels=slice(None), taps=None, edge='zeros', dtype=np.float32):
        """Low-pass filter rows [start, stop) along time and keep every q-th row, on the device: only the output crosses the bus.
        y[k, c] = sum_{j < L} taps[j] * x[start + k * q + half - j, cols[c]] for k < ceil((stop - start) / q), half = (L - 1) // 2,
        computed in `dtype` (float32 or float64): items and taps rounded to it, then acc = acc + taps[j] * x for j = 0 .. L-1 with
        each product and sum rounded -- the same bits whatever the lanes, calls or pieces.  x is 0 outside [start, stop) for
        edge='zeros' (scipy.signal.decimate(x, q, ftype='fir', zero_phase=True, axis=0) when taps is None; resample_poly(x, 1, q,
        window=taps) otherwise) and outside the recording for edge='recording' (pieces then stitch: decimate(q, a, b) followed by
        decimate(q, b, c) is decimate(q, a, c) when (b - a) % q == 0).  taps=None: decimate_taps(q) (q == 1 needs taps); 1 to 8192
        finite taps, used as given.  start / stop follow Reader[...]; channels: an int (the result is then 1-D), a slice with step
        >= 1, or a sequence of ints.  No IIR filters, no rational resampling, no other edge modes.  Chunks resident in the device
        cache are read where they lie; the others are decoded in a transient workspace and NOT kept.  A damaged chunk in the
        support raises the IOError of Reader[...]."""
        self._need_codec('decimate', 'decimate', 'filters')
        if not isinstance(q, (int, np.integer)) or isinstance(q, bool) or q < 1:
            raise ValueError("q must be an int >= 1, got %r" % (q,))
        q = int(q)
        if taps is None:
            if q == 1:
                raise ValueError("decimate(1) needs explicit taps")
            taps = decimate_taps(q)
        taps = _fir_taps(taps)
        out_dtype = _float_dtype(dtype)
        if edge not in ('zeros', 'recording'):
            raise ValueError("edge must be 'zeros' or 'recording', got %r" % (edge,))
        i0, i1 = self._row_range(start, stop)
        cols, squeeze = self._stats_channels(channels)
        n_taps = int(taps.size)
        n_out = -(-(i1 - i0) // q)
        first_row = i0 + (n_taps - 1) // 2
        vb, ve = (i0, i1) if edge == 'zeros' else (0, self.n_samples)
        out = np.zeros((n_out, cols.size), out_dtype)
        lo, hi = max(vb, first_row - (n_taps - 1)), min(ve, first_row + (n_out - 1) * q + 1)
        if n_out and cols.size and lo < hi:
            # calls: cut the outputs where the compressed bytes of the chunks their newest rows lie in pass DECIMATE_CALL_BYTES
            cuts = self._halo_cuts(lo, hi, DECIMATE_CALL_BYTES, 0, n_out, lambda row: min(n_out, max(0, -(-(row - first_row) // q))))

            def part(a, b):
                fr = first_row + a * q
                plo, phi = max(vb, fr - (n_taps - 1)), min(ve, fr + (b - a - 1) * q + 1)
                if plo < phi:                                       # (outputs that read no valid row stay 0)
                    return self._chunk_span(plo, phi), (vb, ve, fr, b - a, q, taps, out_dtype, cols)
            for a, b, (y,) in self._halo_parts(self.codec.decimate, cuts, part):
                out[a:b] = y
        return out[:, 0] if squeeze else out

    # -- channel-mixing matrix products on the device (an extension: the reference's users form Reader[...] @ W on the host)
    def project(self, weights, start=0, stop=None, channels=slice(None), offset=None, dtype=np.float32):
        """Rows [start, stop) times a channel-mixing matrix, on the device: only the result crosses the bus.
        y[t, k] = sum_j (x[t, cols[j]] - offset[j]) * weights[j, k], computed in `dtype` (float32 or float64) on the matrix cores:
        items, offsets and weights are each rounded once to it, the subtraction is one operation, and the sum is the chain of
        4-column matrix steps in column order from +0 -- for float32 bit for bit acc = fmaf(d_j, w_jk, acc) over j, for float64
        within the bound include/mtscomp_hip.h states (gamma_{n+4} * sum_j (|x_j| + |o_j|) |w_jk| plus the underflow term, n the
        columns rounded up to 4).  The same bits whatever the lanes, calls, pieces or cache residency; zero weights are not skipped
        (inf * 0 is NaN).  weights: (n_cols, n_out) finite numbers, n_cols the
        number of selected channels and both at most 1024; 1-D weights mean one output and a 1-D result.  offset: None, a finite
        number or one per column.  Whitening (whitening_weights), projection onto principal components, re-referencing
        (np.eye(n) - 1 / n) and selecting or scaling channels are all this call.  start / stop follow Reader[...]; channels: an
        int (weights then have one row), a slice with step >= 1, or a sequence of ints (repeats allowed).  Returns a (stop -
        start, n_out) array of `dtype`.  Chunks resident in the device cache are read where they lie; the others are decoded in
        a transient workspace and NOT kept.  A damaged chunk raises the IOError of Reader[...]."""
        self._need_codec('project', 'project', 'multiplies')
        out_dtype = _float_dtype(dtype)
        i0, i1 = self._row_range(start, stop)
        cols, _ = self._stats_channels(channels)
        w = np.asarray(weights)
        if w.dtype.kind not in 'fiu' or w.ndim not in (1, 2):
            raise ValueError("weights must be a 1-D or 2-D array of numbers")
        squeeze = w.ndim == 1
        w = np.ascontiguousarray((w[:, None] if squeeze else w).astype(np.float64))
        if w.shape[0] != cols.size:
            raise ValueError("weights have %d rows for %d columns" % (w.shape[0], cols.size))
        if cols.size > hip.PROJECT_MAX_COLS:
            raise ValueError("project takes at most %d columns, got %d" % (hip.PROJECT_MAX_COLS, cols.size))
        if not 1 <= w.shape[1] <= hip.PROJECT_MAX_OUT:
            raise ValueError("project gives 1 to %d outputs, got %d" % (hip.PROJECT_MAX_OUT, w.shape[1]))
        if not np.isfinite(w).all():
            raise ValueError("weights must be finite")
        off = None
        if offset is not None:
            off = np.asarray(offset)
            if off.dtype.kind not in 'fiu' or off.shape not in ((), (cols.size,)):
                raise ValueError("offset must be None, a number or one per column (%d)" % cols.size)
            off = np.ascontiguousarray(np.broadcast_to(off.astype(np.float64), (cols.size,)))
            if not np.isfinite(off).all():
                raise ValueError("offset must be finite")
        n_out = w.shape[1]
        if not (i1 > i0 and cols.size):                            # (nothing to read: no device call)
            out = np.zeros((i1 - i0, n_out), out_dtype)
        else:
            out = np.empty((i1 - i0, n_out), out_dtype)             # (every row is written by a call)
            # calls: cut the rows at the chunk boundaries where the compressed bytes pass PROJECT_CALL_BYTES, and so that a call's
            # result stays within PROJECT_OUT_BYTES
            cuts = self._budget_cuts(i0, i1, PROJECT_CALL_BYTES, i0, i1, n_out * out_dtype.itemsize, PROJECT_OUT_BYTES)

            def part(a, b):
                return self._chunk_span(a, b), (a, b, cols, off, w, out_dtype)
            for a, b, (y,) in self._halo_parts(self.codec.project, cuts, part):
                out[a - i0:b - i0] = y
        return out[:, 0] if squeeze else out

    # -- template scores on the device (an extension: the reference's users filter Reader[...] and run a matched filter on the host)
    def correlate(self, templates, start=0, stop=None, channels=slice(None), before=20, taps=None, reference=None):
        """Spatio-temporal template scores of the filtered rows [start, stop), on the device: only the scores cross the bus.  All in
        float32 on the matrix cores.  z is detect's z: the bytes of decimate(1, taps=taps, edge='recording', dtype=float32) on
        `channels` (taps=None is [1.0]), minus, with reference='median', the float32 median over all selected columns of each row;
        z is +0 outside the recording.  templates: (K, T, W) finite numbers, W the number of selected channels -- the shape of
        waveforms(...).waveforms[e] with neighbours=None, so the mean of a unit's snippets is a template -- each rounded once to
        float32.  Row i of the result is the score with template row `before` laid on file row start + i:
        score[t, k] = sum_tau sum_j z[t - before + tau, j] * templates[k, tau, j], formed bit for bit as acc = fmaf(z, K, acc) from +0
        over the column groups g = 0, 4, 8, .. (outermost; the columns padded with +0 to a multiple of 4), tau = 0 .. T - 1 and the
        four columns of the group (innermost); a NaN score has the bits 0x7fc00000.  Zero template entries are not skipped (inf * 0
        is NaN).  project is the T = 1 case.  The same bytes whatever the other templates, the lanes, calls, pieces, slabs or cache
        residency, and correlate(a, b) followed by correlate(b, c) is correlate(a, c).  1 <= T <= 256, 0 <= before <= T (after = T
        - before is implied), 1 <= K <= 1024, W <= 1024; a 2-D (T, W) array is one template and gives a 1-D result.  start / stop
        follow Reader[...]; channels: an int, a slice with step >= 1, or a sequence of ints (repeats allowed).  Returns a (stop -
        start, K) float32 array.  Chunks resident in the device cache are read where they lie; the others are decoded in a transient
        workspace and NOT kept.  A damaged chunk in the support raises the IOError of Reader[...]."""
        self._need_codec('correlate', 'correlate', 'correlates')
        i0, i1 = self._row_range(start, stop)
        taps, cols, ref_code, (k, squeeze, before) = self._filter_args(
            taps, reference, channels, lambda cols: _template_args(templates, before, cols, 'correlate'))
        (n_out, T, _), n_taps, N = k.shape, int(taps.size), self.n_samples
        out = np.zeros((i1 - i0, n_out), np.float32)
        if i1 > i0:
            def support(a, b):                                      # the file rows that the scores of rows [a, b) read
                return self._support(a, b, 0, before, T - before, n_taps)
            # calls: cut the rows at the chunk boundaries where the compressed bytes of the chunks they read pass CORRELATE_CALL_BYTES,
            # and so that a call's result stays within CORRELATE_OUT_BYTES
            cuts = self._budget_cuts(*support(i0, i1), CORRELATE_CALL_BYTES, i0, i1, 4 * n_out, CORRELATE_OUT_BYTES)

            def part(a, b):
                lo, hi = support(a, b)
                if lo < hi:                                         # (rows that read no row of the recording score +0)
                    return self._chunk_span(lo, hi), (0, N, a, b, taps, cols, ref_code, before, k)
            for a, b, (y,) in self._halo_parts(self.codec.correlate, cuts, part):
                out[a - i0:b - i0] = y
        return out[:, 0] if squeeze else out

    # -- template-matching events on the device (an extension: the reference's users pick the peaks of a matched filter on the host)
    def match_templates(self, templates, threshold, start=0, stop=None, channels=slice(None), before=20, taps=None, reference=None,
                        exclude=None, subtract=None):
        """The peaks of correlate's scores over the rows [start, stop), on the device: only the events cross the bus.  score[t, k] is
        correlate(templates, channels=channels, before=before, taps=taps, reference=reference)'s, bit for bit, for every row t of
        the recording.  (t, k) is an event when score[t, k] > threshold[k] and no score within `exclude` rows (any template, inside
        the recording, inside or outside [start, stop)) beats it: score' > score, or score' == score at an earlier (row, template).
        These are detect's words with every template a neighbour: a NaN score is no event and beats nothing, a plateau gives one
        event (its first row and lowest template), -0 equals +0, of two identical templates the lower index has the event, a row
        has at most one event, and match_templates(a, b) followed by match_templates(b, c) is match_templates(a, c).  templates,
        channels, before, taps and reference as correlate takes them (a 2-D (T, W) array is one template); threshold: a finite
        number or one per template, of any sign; exclude: 0 .. 255 rows, None is min(T - 1, 255) -- no two events closer than a
        template.  Returns a Bunch: sample (int64 file rows, ascending), template (int64), score (float32, the bits of
        correlate(...)[sample - start, template]), threshold (the float32 array used), start, stop, channels, exclude.  The same
        bytes whatever the lanes, calls, pieces, slabs or cache residency.  Chunks resident in the device cache are read where they
        lie; the others are decoded in a transient workspace and NOT kept.  A damaged chunk in the support raises the IOError of
        Reader[...].
        subtract: None, or (sample, template, amplitude) as residual takes them -- the events of an earlier pass with their
        template_amplitudes.  The scores are then correlate's chain, bit for bit, on residual's z' in place of z (for every row of
        the recording, so the calls still stitch with the same list), and the events are the peaks that the subtracted templates
        hid: a spike within `exclude` rows of a stronger one."""
        self._need_codec('match_templates', 'match_templates', 'matches templates')
        if subtract is not None:
            self._need_codec('match_templates(subtract=)', 'match_residual', 'subtracts templates')
            if not isinstance(subtract, (tuple, list)) or len(subtract) != 3:
                raise ValueError("subtract must be None or (sample, template, amplitude)")
        i0, i1 = self._row_range(start, stop)
        taps, cols, ref_code, (k, _, before) = self._filter_args(
            taps, reference, channels, lambda cols: _template_args(templates, before, cols, 'match_templates'))
        n_out, T, _ = k.shape
        if exclude is None:
            exclude = min(T - 1, hip.TMATCH_MAX_EXCLUDE)
        if not isinstance(exclude, (int, np.integer)) or isinstance(exclude, bool) or not 0 <= exclude <= hip.TMATCH_MAX_EXCLUDE:
            raise ValueError("exclude must be an int in [0, %d], got %r" % (hip.TMATCH_MAX_EXCLUDE, exclude))
        thr = np.asarray(threshold)
        if thr.dtype.kind not in 'fiu' or thr.shape not in ((), (n_out,)):
            raise ValueError("threshold must be a number or one per template (%d)" % n_out)
        with np.errstate(over='ignore'):
            thr = np.ascontiguousarray(np.broadcast_to(thr.astype(np.float32), (n_out,)))
        if not np.isfinite(thr).all():
            raise ValueError("threshold must be finite in float32")
        R, n_taps, N, after = int(exclude), int(taps.size), self.n_samples, T - before
        sub = None if subtract is None else _sub_events(*subtract, n_out, N)
        found = []                                                  # (row, template, score) of every part, in order
        if i1 > i0:
            def support(a, b):                                      # the file rows that the events of rows [a, b) read
                return self._support(a, b, R, before, after, n_taps)
            # calls: cut the rows at the chunk boundaries where the compressed bytes of the chunks they read pass TMATCH_CALL_BYTES
            lo, hi = support(i0, i1)
            cuts = self._halo_cuts(lo, hi, TMATCH_CALL_BYTES, i0, i1, lambda row: min(i1, max(i0, row))) if lo < hi else [i0, i1]

            def part(a, b):
                lo, hi = support(a, b)                              # (rows that read no row of the recording score +0: a call without chunks)
                keys = self._chunk_span(lo, hi) if lo < hi else []
                cap = max(TMATCH_GUESS_MIN, (b - a) // TMATCH_GUESS_SAMPLES)
                args = (0, N, a, b, taps, cols, ref_code, before, k, thr, R, cap)          # (cap at _TMATCH_CAP_AT)
                if sub is None:
                    return keys, args
                # with every event whose window meets the rows that the call computes z for: [a - R - before, b + R + after - 1)
                e0, e1 = np.searchsorted(sub[0], [a - R - T + 1, b + R + after - 1 + before])
                return keys, args + tuple(v[e0:e1] for v in sub)

            fn = self.codec.match_templates if sub is None else self.codec.match_residual
            found = [ev[1:] for _, _, ev in self._halo_parts(fn, cuts, part, _again_with_room(_TMATCH_CAP_AT))]
        row, tpl, val = _event_arrays(found)
        return Bunch(sample=row, template=tpl, score=val, threshold=thr, start=i0, stop=i1, channels=cols, exclude=R)

    # -- template peeling on the device (an extension: the reference's users subtract matched templates from Reader[...] on the host)
    def residual(self, sample, template, amplitude, templates, start=0, stop=None, channels=slice(None), before=20, taps=None, reference=None):
        """The filtered rows [start, stop) with matched templates subtracted, on the device.  All in float32.  z is correlate's z
        inside the recording: the bytes of decimate(1, taps=taps, edge='recording', dtype=float32) on `channels` (taps=None is
        [1.0]), minus, with reference='median', the float32 median over all selected columns of each row.  The events (sample[e],
        template[e], amplitude[e]) -- 1-D arrays of one length, 0 <= sample < n_samples in any order with repeats, template an index
        into `templates`, amplitude finite -- are ordered by sample, equal samples in list order.  Event e covers file row t when 0 <=
        tau = t - sample[e] + before < T, and row i of the result is, for t = start + i,
        acc = z[t, j]; for every event that covers t, in that order: acc = fmaf(-amplitude[e], templates[template[e], tau, j], acc),
        bit for bit; a NaN has the bits 0x7fc00000.  An event that does not cover a row does nothing to it (no masked step: -0
        stays -0), zero template entries are not skipped, and an empty list returns z itself -- the referenced, filtered rows.
        The same bytes whatever the lanes, calls, pieces, slabs, cache residency or the events that cover none of the rows asked
        for, and residual(a, b) followed by residual(b, c) is residual(a, c).  templates, channels, before, taps and reference as
        correlate takes them (a 2-D (T, W) array is one template).  With ev = match_templates(K, thr) and amp =
        template_amplitudes(ev.score, ev.template, K), residual(ev.sample, ev.template, amp, K) is what a second pass,
        match_templates(K, thr, subtract=(ev.sample, ev.template, amp)), scores.  start / stop follow Reader[...].  Returns a (stop
        - start, W) float32 array.  Chunks resident in the device cache are read where they lie; the others are decoded in a
        transient workspace and NOT kept.  A damaged chunk in the support raises the IOError of Reader[...]."""
        self._need_codec('residual', 'residual', 'subtracts templates')
        i0, i1 = self._row_range(start, stop)
        taps, cols, ref_code, (k, _, before) = self._filter_args(
            taps, reference, channels, lambda cols: _template_args(templates, before, cols, 'residual'))
        (n_out, T, W), n_taps, N = k.shape, int(taps.size), self.n_samples
        sub = _sub_events(sample, template, amplitude, n_out, N)
        out = np.empty((i1 - i0, W), np.float32)                    # (every row is inside the recording and written by a call)
        if i1 > i0:
            def support(a, b):                                      # the file rows that rows [a, b) read: their filter support
                return self._support(a, b, 0, 0, 1, n_taps)
            # calls: cut the rows at the chunk boundaries where the compressed bytes of the chunks they read pass RESIDUAL_CALL_BYTES,
            # and so that a call's result stays within RESIDUAL_OUT_BYTES
            cuts = self._budget_cuts(*support(i0, i1), RESIDUAL_CALL_BYTES, i0, i1, 4 * W, RESIDUAL_OUT_BYTES)

            def part(a, b):
                # with every event whose window [sample - before, sample - before + T) meets the rows [a, b)
                e0, e1 = np.searchsorted(sub[0], [a + before - T + 1, b + before])
                return self._chunk_span(*support(a, b)), (0, N, a, b, taps, cols, ref_code, before, k) + tuple(v[e0:e1] for v in sub)
            for a, b, (y,) in self._halo_parts(self.codec.residual, cuts, part):
                out[a - i0:b - i0] = y
        return out

    # -- peak detection on the device (an extension: the reference's users filter Reader[...] and look for peaks on the host)
    def detect(self, threshold, start=0, stop=None, channels=slice(None), taps=None, sign='neg', reference=None, exclude=0, spread=0):
        """Threshold crossings of the filtered rows [start, stop), on the device: only the events cross the bus.  All in float32:
        y[t, j] = sum_{k < L} taps[k] * x[t + half - k, cols[j]], half = (L - 1) // 2, x = 0 outside the recording -- the bytes of
        decimate(1, taps=taps, edge='recording', dtype=float32); taps=None is [1.0], highpass_taps(300, sample_rate) the spike band.
        reference='median': z = y - the median over the selected columns of row t (np.sort's order; 0.5 * (a + b) for an even
        number; NaN if the row holds one), else z = y.  v = -z (sign='neg'), z ('pos') or |z| ('both').  (t, j) is an event when
        v > threshold[j] and no neighbour within `exclude` rows and `spread` column positions (positions in `channels`, inside the
        recording, inside or outside [start, stop)) beats it: v' > v, or v' == v at an earlier (t, j).  So a plateau gives one event,
        NaN none, and detect(a, b) followed by detect(b, c) is detect(a, c).  threshold: a positive finite number or one per column
        (5 * mad(...).mad / 0.6745 is the usual choice).  Returns a Bunch: sample (int64 file rows), channel (int64, the entries of
        `channels`), amplitude (float32 z, signed), in ascending (sample, position) order; threshold (the float32 array used), start,
        stop, channels.  start / stop follow Reader[...]; channels: an int, a slice with step >= 1, or a sequence of ints (repeats
        allowed).  exclude <= 255, spread <= 32, a median over at most 1024 columns.  The same bytes whatever the lanes, calls,
        pieces or cache residency.  Chunks resident in the device cache are read where they lie; the others are decoded in a
        transient workspace and NOT kept.  A damaged chunk in the support raises the IOError of Reader[...]."""
        self._need_codec('detect', 'detect', 'detects')
        if sign not in hip.DETECT_SIGNS:
            raise ValueError("sign must be 'neg', 'pos' or 'both', got %r" % (sign,))
        for name, v, top in (('exclude', exclude, hip.DETECT_MAX_EXCLUDE), ('spread', spread, hip.DETECT_MAX_SPREAD)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= v <= top:
                raise ValueError("%s must be an int in [0, %d], got %r" % (name, top, v))
        i0, i1 = self._row_range(start, stop)

        def thresholds(cols):
            thr = np.asarray(threshold)
            if thr.dtype.kind not in 'fiu' or thr.shape not in ((), (cols.size,)):
                raise ValueError("threshold must be a number or one per column (%d)" % cols.size)
            with np.errstate(over='ignore'):
                thr = np.ascontiguousarray(np.broadcast_to(thr.astype(np.float32), (cols.size,)))
            if not (np.isfinite(thr) & (thr > 0)).all():
                raise ValueError("threshold must be positive and finite in float32")
            return thr
        taps, cols, ref_code, thr = self._filter_args(taps, reference, channels, thresholds)
        R, S, n_taps, N, sign_code = int(exclude), int(spread), int(taps.size), self.n_samples, hip.DETECT_SIGNS[sign]
        found = []                                                  # (row, pos, amp) of every part, in order
        if i1 > i0 and cols.size:
            # calls: cut the rows at the chunk boundaries where the compressed bytes of the chunks they lie in pass DETECT_CALL_BYTES
            cuts = self._halo_cuts(i0, i1, DETECT_CALL_BYTES, i0, i1, lambda row: row)

            def part(a, b):
                keys = self._chunk_span(*self._support(a, b, R, 0, 1, n_taps))
                cap = max(DETECT_GUESS_MIN, (b - a) * cols.size // DETECT_GUESS_SAMPLES)
                return keys, (0, N, a, b, taps, cols, thr, sign_code, ref_code, R, S, cap)     # (cap at _DETECT_CAP_AT)
            found = [ev[1:] for _, _, ev in self._halo_parts(self.codec.detect, cuts, part, _again_with_room(_DETECT_CAP_AT))]
        row, pos, amp = _event_arrays(found)
        return Bunch(sample=row, channel=cols.astype(np.int64)[pos], amplitude=amp, threshold=thr, start=i0, stop=i1, channels=cols)

    # -- snippets around events on the device (an extension: the reference's users filter Reader[...] and slice it on the host)
    def _waveform_cuts(self, lo, hi, max_bytes, max_events):
        """The calls of waveforms: the events (by ascending row; event i reads file rows [lo[i], hi[i])) cut where consecutive
        events' chunk spans leave at least one whole chunk unread, where the compressed bytes of a call's chunks pass max_bytes,
        and so that a call holds at most max_events.  -> the cut list, 0 first, the number of events last."""
        n = int(lo.size)
        bounds = np.asarray(self.chunk_bounds, dtype=np.int64)
        k_lo = np.searchsorted(bounds, lo, side='right') - 1
        k_hi = np.searchsorted(bounds, hi - 1, side='right') - 1
        # the spans ascend with the events: only an event whose span differs from the one before it can start a call

        def nbytes(a, b):
            return self.chunk_offsets[b + 1] - self.chunk_offsets[a] if b >= a else 0
        base, acc, top = [0], 0, -1                                 # top: the last chunk of the call so far
        for i in np.concatenate(([0], np.flatnonzero((np.diff(k_lo) != 0) | (np.diff(k_hi) != 0)) + 1)).tolist():
            a, b = int(k_lo[i]), int(k_hi[i])
            new = nbytes(max(a, top + 1), b)
            if i and (a > top + 1 or (new and acc + new > max_bytes)):
                base.append(i)
                acc, top, new = 0, -1, nbytes(a, b)
            acc, top = acc + new, max(top, b)
        base.append(n)
        return [u for a, b in zip(base[:-1], base[1:]) for u in range(a, b, max_events)] + [n]

    def _snippet_args(self, what, sample, channel, before, after, neighbours, channels, taps, reference):
        """The arguments that waveforms, mean_waveforms, waveform_features and localize share, checked -> (before, after, T, W, taps, cols, reference code, the
        events' rows as int64, their first positions)."""
        for name, v in (('before', before), ('after', after)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 0:
                raise ValueError("%s must be an int >= 0, got %r" % (name, v))
        before, after = int(before), int(after)
        T = before + after
        if not 1 <= T <= hip.WAVEFORMS_MAX_ROWS:
            raise ValueError("before + after must be in [1, %d], got %d" % (hip.WAVEFORMS_MAX_ROWS, T))
        if neighbours is not None and (not isinstance(neighbours, (int, np.integer)) or isinstance(neighbours, bool) or neighbours < 0):
            raise ValueError("neighbours must be None or an int >= 0, got %r" % (neighbours,))
        def width(cols):
            if not cols.size:
                raise ValueError("%s needs at least one channel" % what)
            W = int(cols.size) if neighbours is None else 2 * int(neighbours) + 1
            if W > hip.WAVEFORMS_MAX_WIDTH:
                raise ValueError("a snippet holds at most %d positions, got %d" % (hip.WAVEFORMS_MAX_WIDTH, W))
            return W
        taps, cols, ref_code, W = self._filter_args(taps, reference, channels, width)
        rows = np.asarray(sample)
        if rows.ndim != 1 or (rows.size and rows.dtype.kind not in 'iu'):
            raise ValueError("sample must be a 1-D array of ints")
        rows = rows.astype(np.int64)
        n, N = int(rows.size), self.n_samples
        if n and (rows.min() < 0 or rows.max() >= N):
            raise ValueError("sample must lie in [0, %d)" % N)
        if neighbours is None:
            col0 = np.zeros(n, np.int64)
        else:
            if channel is None:
                raise ValueError("neighbours=%d needs the events' channels" % neighbours)
            ch = np.asarray(channel)
            if ch.shape != rows.shape or (ch.size and ch.dtype.kind not in 'iu'):
                raise ValueError("channel must hold one int per sample")
            ch = ch.astype(np.int64)
            first = np.full(self.n_channels, -1, np.int64)          # the first position in `channels` of every file channel
            first[cols[::-1]] = np.arange(cols.size - 1, -1, -1)
            if n and (ch.min() < 0 or ch.max() >= self.n_channels or (first[ch] < 0).any()):
                raise ValueError("channel holds a channel that is not among `channels`")
            col0 = first[ch] - int(neighbours)
        return before, after, T, W, taps, cols, ref_code, rows, col0

    def waveforms(self, sample, channel=None, before=20, after=41, neighbours=None, channels=slice(None), taps=None, reference=None,
                  waveforms=True):
        """Snippets of the filtered rows around events, and their extrema, on the device: only they cross the bus.  All in float32.
        z is detect's z: the bytes of decimate(1, taps=taps, edge='recording', dtype=float32) on `channels` (taps=None is [1.0]),
        minus, with reference='median', the float32 median over all selected columns of each row.  Event e at file row sample[e]:
        waveforms[e, tau, w] = z[sample[e] - before + tau, position[e] + w] for tau < T = before + after and w < W.
        neighbours=None: W is the number of selected channels and position 0 (`channel` is not needed); neighbours=k >= 0: W =
        2 k + 1 and position[e] = pos - k, pos the first position in `channels` that holds channel[e] (file channel numbers, as
        detect returns them; a channel that is not selected is a ValueError).  An entry whose row lies outside the recording or
        whose position lies outside the selection is NaN (every NaN entry, fill or data, has the bits 0x7fc00000).  trough / peak: the minimum / maximum over the entries that are not NaN
        (the first one in (tau, w) order; -0 == +0), each a Bunch of value (float32; NaN for none), offset (int64, tau - before; 0
        for none), channel (int64, the entry of `channels`; -1 for none) and index (int64, tau * W + w; -1 for none).  So
        waveforms[e, before, pos - position[e]] is detect's amplitude of the event, bit for bit.  sample: ints in [0, n_samples),
        any order, repeats allowed; the results come in that order.  waveforms=False: the extrema alone (the same bytes),
        `waveforms` is None.  Returns a Bunch: waveforms (n, T, W), trough, peak, sample, position, before, after, channels.  T <=
        4096, W <= 1024, a median over at most 1024 columns.  The same bytes whatever the lanes, calls, pieces or cache residency.
        Only the chunks that the events' snippets and their filter support read are decoded: resident chunks are read where they
        lie, the others in a transient workspace and NOT kept.  A damaged chunk in an event's support raises the IOError of
        Reader[...]."""
        self._need_codec('waveforms', 'waveforms', 'gathers')
        before, after, T, W, taps, cols, ref_code, rows, col0 = self._snippet_args('waveforms', sample, channel, before, after, neighbours, channels,
                                                                                  taps, reference)
        n, N = int(rows.size), self.n_samples
        order = np.argsort(rows, kind='stable')
        s_rows, s_col0 = rows[order], col0[order]
        n_taps = int(taps.size)
        half = (n_taps - 1) // 2
        wave = np.empty((n, T, W), np.float32) if waveforms else None
        ext = [np.empty(n, t) for t in (np.float32, np.int64, np.float32, np.int64)]
        if n:
            lo = np.maximum(0, s_rows - before + half - (n_taps - 1))  # the file rows an event reads
            hi = np.minimum(N, s_rows + after + half)
            cuts = self._waveform_cuts(lo, hi, WAVEFORMS_CALL_BYTES, max(1, WAVEFORMS_OUT_BYTES // (4 * T * W + 16)))

            def part(a, b):
                return (self._chunk_span(int(lo[a]), int(hi[b - 1])),
                        (0, N, taps, cols, ref_code, s_rows[a:b], s_col0[a:b], before, after, W, bool(waveforms)))
            in_order = bool((order[1:] > order[:-1]).all())          # (detect's events are: plain copies then)
            for a, b, got in self._halo_parts(self.codec.waveforms, cuts, part):
                where = slice(a, b) if in_order else order[a:b]
                if waveforms:
                    wave[where] = got[0]
                for dst, src in zip(ext, got[1:]):
                    dst[where] = src
        out = {}
        for name, value, index in (('trough', ext[0], ext[1]), ('peak', ext[2], ext[3])):
            some = index >= 0
            pos = np.where(some, col0 + index % W, 0)
            out[name] = Bunch(value=value, offset=np.where(some, index // W - before, 0), channel=np.where(some, cols[pos], -1), index=index)
        return Bunch(waveforms=wave, trough=out['trough'], peak=out['peak'], sample=rows, position=col0, before=before, after=after,
                     channels=cols)

    # -- per-unit mean snippets on the device (an extension: the reference's users average the snippets on the host)
    def mean_waveforms(self, sample, label, channel=None, before=20, after=41, neighbours=None, channels=slice(None), taps=None, reference=None,
                       n_labels=None, resolution=2.0 ** -16):
        """The mean snippet of every label (a unit's template), summed on the device in fixed point: K * T * W numbers cross the
        bus, not one snippet per event.  sample, channel, neighbours, channels, taps, reference, before and after mean what they
        mean for `waveforms`; label holds one int per sample, events with label < 0 are ignored (the usual noise cluster); n_labels
        = K, None: max(label) + 1.  sample may come in any order.  Over the entries (e, tau, w) of waveforms(...).waveforms that are
        not fill entries, with d = float64(entry) / resolution (resolution a power of two in [2^-60, 2^60]: exact): a NaN entry or
        |d| >= 2^42 adds 1 to skipped[label[e]]; every other adds rint(d) (ties to even) to sum[label[e], tau, w] and 1 to
        count[label[e], tau, w].  Returns a Bunch: mean (K, T, W) float32 = float32(float64(sum) * resolution / count), NaN (bits
        0x7fc00000) where count is 0; sum, count (K, T, W) int64; skipped (K) int64; events (K) int64, the events of each label;
        resolution, before, after, channels.  Integer sums do not depend on the order: the same bytes whatever the order of sample,
        the lanes, calls, pieces or cache residency, and equal to the sums formed from waveforms' own snippets.  With
        neighbours=None, np.nan_to_num(mean) is a valid `templates` argument of correlate and match_templates.  At most 2^21 events
        of one label, K <= 4096, K * T * W <= 2^27; T, W and the median's columns as waveforms.  Chunks are read as waveforms reads
        them, and a damaged chunk in an event's support raises the IOError of Reader[...]."""
        self._need_codec('mean_waveforms', 'mean_waveforms', 'sums snippets')
        before, after, T, W, taps, cols, ref_code, rows, col0 = self._snippet_args('mean_waveforms', sample, channel, before, after, neighbours,
                                                                                  channels, taps, reference)
        lab = np.asarray(label)
        if lab.shape != rows.shape or (lab.size and lab.dtype.kind not in 'iu'):
            raise ValueError("label must hold one int per sample")
        lab = lab.astype(np.int64)
        top = int(lab.max()) + 1 if lab.size else 0
        if n_labels is None:
            n_labels = max(top, 0)
        elif not isinstance(n_labels, (int, np.integer)) or isinstance(n_labels, bool) or n_labels < 0:
            raise ValueError("n_labels must be None or an int >= 0, got %r" % (n_labels,))
        K = int(n_labels)
        if top > K:
            raise ValueError("label holds %d, n_labels is %d" % (top - 1, K))
        if K > hip.MEAN_MAX_LABELS or K * T * W > hip.MEAN_MAX_ENTRIES:
            raise ValueError("at most %d labels and %d sums (labels x rows x positions), got %d and %d"
                             % (hip.MEAN_MAX_LABELS, hip.MEAN_MAX_ENTRIES, K, K * T * W))
        if not isinstance(resolution, (int, float, np.integer, np.floating)) or isinstance(resolution, bool) or not hip.mean_resolution_ok(resolution):
            raise ValueError("resolution must be a power of two in [2^-60, 2^60], got %r" % (resolution,))
        resolution = float(resolution)
        keep = lab >= 0
        rows, col0, lab = rows[keep], col0[keep], lab[keep]
        events = np.bincount(lab, minlength=K).astype(np.int64)
        if events.size and int(events.max()) > hip.MEAN_MAX_LABEL_EVENTS:
            raise ValueError("label %d has %d events (at most %d)" % (int(events.argmax()), int(events.max()), hip.MEAN_MAX_LABEL_EVENTS))
        total, count, skipped = np.zeros((K, T, W), np.int64), np.zeros((K, T, W), np.int64), np.zeros(K, np.int64)
        n, N = int(rows.size), self.n_samples
        if n:
            order = np.argsort(rows, kind='stable')
            s_rows, s_col0, s_lab = rows[order], col0[order], lab[order]
            n_taps = int(taps.size)
            half = (n_taps - 1) // 2
            lo = np.maximum(0, s_rows - before + half - (n_taps - 1))  # the file rows an event reads
            hi = np.minimum(N, s_rows + after + half)
            cuts = self._waveform_cuts(lo, hi, WAVEFORMS_CALL_BYTES, max(1, MEAN_WAVEFORMS_EVENT_BYTES // 24))

            def part(a, b):
                return (self._chunk_span(int(lo[a]), int(hi[b - 1])),
                        (0, N, taps, cols, ref_code, s_rows[a:b], s_col0[a:b], s_lab[a:b], K, before, after, W, resolution))
            for _, _, (s, c, k) in self._halo_parts(self.codec.mean_waveforms, cuts, part):     # (integers: any cut adds up to the same)
                total += s
                count += c
                skipped += k
        with np.errstate(divide='ignore', invalid='ignore'):
            mean = (total.astype(np.float64) * resolution / count).astype(np.float32)
        mean[count == 0] = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]
        return Bunch(mean=mean, sum=total, count=count, skipped=skipped, events=events, resolution=resolution, before=before, after=after,
                     channels=cols)

    # -- snippets projected on a temporal basis on the device (an extension: the reference's users run an einsum on the snippets)
    def waveform_features(self, sample, basis, channel=None, before=20, after=41, neighbours=None, channels=slice(None), taps=None,
                          reference=None):
        """The snippets of `waveforms` projected on a small temporal basis -- the "PC features" that clustering reads -- on the
        device: P numbers of every T cross the bus.  sample, channel, neighbours, channels, taps, reference, before and after mean
        what they mean for `waveforms`.  basis: (P, T) numbers, T = before + after (api.waveform_basis makes one from snippets),
        rounded once to float32; every entry must be finite, also after the rounding.  All in float32, with s =
        waveforms(...).waveforms: features[e, p, w] is the chain acc = +0; for tau = 0 .. T - 1: acc = fmaf(s[e, tau, w],
        basis[p, tau], acc), bit for bit; every NaN result has the bits 0x7fc00000.  Zero basis entries are not skipped (inf * 0 is
        NaN), so one NaN entry -- fill or data -- in the column s[e, :, w] makes features[e, :, w] NaN: an event near the
        recording's ends is NaN throughout, a position outside the selection is NaN for its events.  A 1-D basis (T,) gives features
        (n, W), without the P axis.  sample: ints in [0, n_samples), any order, repeats allowed; the results come in that order.
        Returns a Bunch: features (n, P, W) float32, sample, position, basis (the float32 (P, T) array used), before, after,
        channels.  P <= 32, P * T <= 8192; T, W and the median's columns as waveforms.  The same bytes whatever the order of sample,
        the lanes, calls, pieces or cache residency, and the bytes of that chain run on the host over waveforms' own snippets.
        Chunks are read as waveforms reads them, and a damaged chunk in an event's support raises the IOError of Reader[...]."""
        self._need_codec('waveform_features', 'waveform_features', 'projects snippets')
        before, after, T, W, taps, cols, ref_code, rows, col0 = self._snippet_args('waveform_features', sample, channel, before, after,
                                                                                  neighbours, channels, taps, reference)
        b = np.asarray(basis)
        if b.dtype.kind not in 'fiu' or b.ndim not in (1, 2) or b.shape[-1] != T:
            raise ValueError("basis must be a (P, %d) or (%d,) array of numbers (before + after = %d), got shape %r" % (T, T, T, b.shape))
        flat = b.ndim == 1
        with np.errstate(over='ignore'):
            b = np.ascontiguousarray(np.atleast_2d(b).astype(np.float32))
        P = int(b.shape[0])
        if not 1 <= P <= hip.FEATURES_MAX_COMPONENTS or P * T > hip.FEATURES_MAX_BASIS:
            raise ValueError("at most %d components and %d basis entries (components x rows), got %d and %d"
                             % (hip.FEATURES_MAX_COMPONENTS, hip.FEATURES_MAX_BASIS, P, P * T))
        if not np.isfinite(b).all():
            raise ValueError("basis must be finite as float32")
        n, N = int(rows.size), self.n_samples
        feat = np.empty((n, P, W), np.float32)
        if n:
            order = np.argsort(rows, kind='stable')
            s_rows, s_col0 = rows[order], col0[order]
            n_taps = int(taps.size)
            half = (n_taps - 1) // 2
            lo = np.maximum(0, s_rows - before + half - (n_taps - 1))  # the file rows an event reads
            hi = np.minimum(N, s_rows + after + half)
            cuts = self._waveform_cuts(lo, hi, WAVEFORMS_CALL_BYTES, max(1, WAVEFORMS_OUT_BYTES // (4 * P * W)))

            def part(a, b_):
                return (self._chunk_span(int(lo[a]), int(hi[b_ - 1])),
                        (0, N, taps, cols, ref_code, s_rows[a:b_], s_col0[a:b_], before, after, W, b))
            in_order = bool((order[1:] > order[:-1]).all())          # (detect's events are: plain copies then)
            for a, b_, got in self._halo_parts(self.codec.waveform_features, cuts, part):
                feat[slice(a, b_) if in_order else order[a:b_]] = got[0]
        return Bunch(features=feat[:, 0] if flat else feat, sample=rows, position=col0, basis=b, before=before, after=after, channels=cols)

    # -- spike positions and channel amplitudes on the device (an extension: the reference's users reduce the snippets on the host)
    def localize(self, sample, positions, channel=None, before=20, after=41, neighbours=None, channels=slice(None), taps=None,
                 reference=None, amplitude='ptp', amplitudes=True):
        """Where on the probe every spike happened -- the amplitude-weighted mean of the channel positions, the "centre of mass"
        of drift maps and motion estimation -- and its amplitude on every channel of the snippet, on the device: W + D + 2 numbers
        an event cross the bus, not T * W.  sample, channel, neighbours, channels, taps, reference, before and after mean what they
        mean for `waveforms`.  positions: (n_selected, D) numbers, 1 <= D <= 4, the probe geometry in the caller's units, one row
        per entry of `channels` in selection order (not per file channel), rounded once to float32; every entry must be finite,
        also after the rounding.  A 1-D positions (n_selected,) is D = 1 and gives location and moment without the D axis.
        amplitude: 'ptp', 'neg', 'pos' or 'abs'.  All in float32 and bit for bit, with s = waveforms(...).waveforms: over the
        entries s[e, tau, w], tau = 0 .. T - 1, that are not NaN, lo is the first minimum and hi the first maximum (-0 == +0: the
        first wins); amplitude[e, w] is hi - lo ('ptp', one subtraction), -lo ('neg'; +0 gives -0), hi ('pos') or the first maximum
        of abs(entry) ('abs'), and NaN (every NaN has the bits 0x7fc00000) for a column without such an entry -- a position outside
        the selection, an event whose rows all lie outside the recording, all-NaN data -- and for a NaN result.  NaN entries are
        skipped (waveforms' extrema rule, not waveform_features' contamination rule): a spike near the recording's ends keeps the
        amplitudes of the rows it has.  g[e, w] = amplitude[e, w] where that is > 0, else +0.  One chain per event over w = 0 ..
        W - 1 in ascending order, c = position[e] + w, a w with c outside the selection left out, from +0: weight = weight +
        g[e, w] (one addition), moment[d] = fmaf(g[e, w], positions[c, d], moment[d]) (one fmaf); a step with g = +0 changes no bit
        whether taken or not.  best[e] is the lowest w whose amplitude is the largest among those that are not NaN, -1 for none.
        location[e, d] = float32(float64(moment[e, d]) / float64(weight[e])), formed on the host, NaN where weight is 0 or the
        quotient is NaN.  sample: ints in [0, n_samples), any order, repeats allowed; the results come in that order.  Returns a
        Bunch: location (n, D) float32, amplitude (n, W) float32 (None with amplitudes=False; everything else is the same bytes),
        weight (n) float32, moment (n, D) float32, best (n) int64, channel (n) int64 (the entry of `channels` at position + best,
        -1 for none), sample, position, positions (the float32 (n_selected, D) array used), before, after, channels, mode.  The
        same bytes whatever the order of sample, the lanes, calls, pieces or cache residency, and the bytes of the definition run
        on the host over waveforms' own snippets.  T, W and the median's columns as waveforms.  Chunks are read as waveforms reads
        them, and a damaged chunk in an event's support raises the IOError of Reader[...]."""
        self._need_codec('localize', 'localize', 'localizes spikes')
        before, after, T, W, taps, cols, ref_code, rows, col0 = self._snippet_args('localize', sample, channel, before, after, neighbours,
                                                                                  channels, taps, reference)
        if not isinstance(amplitude, str) or amplitude not in hip.LOCALIZE_MODES:
            raise ValueError("amplitude must be 'ptp', 'neg', 'pos' or 'abs', got %r" % (amplitude,))
        mode = hip.LOCALIZE_MODES[amplitude]
        p = np.asarray(positions)
        if p.dtype.kind not in 'fiu' or p.ndim not in (1, 2) or p.shape[0] != cols.size:
            raise ValueError("positions must be a (%d, D) or (%d,) array of numbers, one row per selected channel, got shape %r"
                             % (cols.size, cols.size, p.shape))
        flat = p.ndim == 1
        with np.errstate(over='ignore'):
            p = np.ascontiguousarray(p.reshape(cols.size, -1).astype(np.float32))
        D = int(p.shape[1])
        if not 1 <= D <= hip.LOCALIZE_MAX_DIMS:
            raise ValueError("positions must have 1 to %d coordinates a channel, got %d" % (hip.LOCALIZE_MAX_DIMS, D))
        if not np.isfinite(p).all():
            raise ValueError("positions must be finite as float32")
        n, N = int(rows.size), self.n_samples
        amp = np.empty((n, W), np.float32) if amplitudes else None
        weight, moment, best = np.empty(n, np.float32), np.empty((n, D), np.float32), np.empty(n, np.int64)
        if n:
            order = np.argsort(rows, kind='stable')
            s_rows, s_col0 = rows[order], col0[order]
            n_taps = int(taps.size)
            half = (n_taps - 1) // 2
            lo = np.maximum(0, s_rows - before + half - (n_taps - 1))  # the file rows an event reads
            hi = np.minimum(N, s_rows + after + half)
            cuts = self._waveform_cuts(lo, hi, WAVEFORMS_CALL_BYTES, max(1, WAVEFORMS_OUT_BYTES // (4 * (W + D + 2))))

            def part(a, b):
                return (self._chunk_span(int(lo[a]), int(hi[b - 1])),
                        (0, N, taps, cols, ref_code, s_rows[a:b], s_col0[a:b], before, after, W, mode, p, bool(amplitudes)))
            in_order = bool((order[1:] > order[:-1]).all())          # (detect's events are: plain copies then)
            for a, b, got in self._halo_parts(self.codec.localize, cuts, part):
                where = slice(a, b) if in_order else order[a:b]
                if amplitudes:
                    amp[where] = got[0]
                weight[where], moment[where], best[where] = got[1], got[2], got[3]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            location = (moment.astype(np.float64) / weight.astype(np.float64)[:, None]).astype(np.float32)
        location[np.isnan(location) | (weight == 0)[:, None]] = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]
        some = best >= 0
        chan = np.where(some, cols[np.where(some, col0 + best, 0)], -1)
        return Bunch(location=location[:, 0] if flat else location, amplitude=amp, weight=weight, moment=moment[:, 0] if flat else moment,
                     best=best, channel=chan, sample=rows, position=col0, positions=p, before=before, after=after, channels=cols, mode=amplitude)

    # -- power spectral density on the device (an extension: the reference's users run scipy.signal.welch on Reader[...])
    def welch(self, nperseg=256, start=0, stop=None, channels=slice(None), noverlap=None, window='hann', detrend='constant',
              scaling='density', dtype=np.float32):
        """Per-channel power spectral density of rows [start, stop) by Welch's method, on the device: only the partial sums cross
        the bus.  Returns (f, psd): f = np.fft.rfftfreq(nperseg, 1 / sample_rate), psd float64 of shape (nperseg // 2 + 1, n_cols)
        (1-D when channels is an int).  With the defaults this is scipy.signal.welch(self[start:stop, channels], fs=sample_rate,
        nperseg=nperseg, axis=0) up to rounding; so it is for the other noverlap, window, detrend and scaling values.
        nperseg: a power of two in [16, 16384] (the FFT length; no nfft).  noverlap: None (nperseg // 2) or 0 <= noverlap < nperseg;
        segment k covers rows [start + k * step, + nperseg), step = nperseg - noverlap, for k < (n - nperseg) // step + 1 (n = stop -
        start; rows after the last whole segment are not used).  window: 'hann', 'hamming', 'boxcar' (scipy's periodic windows) or
        nperseg finite numbers.  detrend: 'constant' (the segment's mean, in float64) or False.  scaling: 'density' (1 / (fs *
        sum w^2)) or 'spectrum' (1 / (sum w)^2); bins other than 0 and nperseg / 2 are doubled.  dtype: the FFT's compute type,
        float32 or float64.  start / stop follow Reader[...]; channels: an int, a slice with step >= 1, or a sequence of ints
        (repeats allowed).  Unlike scipy, a range shorter than nperseg is a ValueError (scipy shrinks nperseg).  The result of a
        column does not depend on the lanes, calls, pieces, cache residency or the other columns (the summation tree depends on
        (nperseg, step, dtype) only).  Chunks resident in the device cache are read where they lie; the others are decoded in a
        transient workspace and NOT kept.  A damaged chunk among the rows read raises the IOError of Reader[...]."""
        self._need_codec('welch', 'welch', 'computes spectra')
        if (not isinstance(nperseg, (int, np.integer)) or isinstance(nperseg, bool) or not 16 <= nperseg <= hip.WELCH_MAX_NPERSEG
                or nperseg & (nperseg - 1)):
            raise ValueError("nperseg must be a power of two in [16, %d], got %r" % (hip.WELCH_MAX_NPERSEG, nperseg))
        nperseg = int(nperseg)
        if noverlap is None:
            noverlap = nperseg // 2
        if not isinstance(noverlap, (int, np.integer)) or isinstance(noverlap, bool) or not 0 <= noverlap < nperseg:
            raise ValueError("noverlap must be None or an int in [0, nperseg), got %r" % (noverlap,))
        step = nperseg - int(noverlap)
        taper = welch_window(window, nperseg)
        if detrend is False:
            dt = False
        elif isinstance(detrend, str) and detrend == 'constant':
            dt = True
        else:
            raise ValueError("detrend must be 'constant' or False, got %r" % (detrend,))
        if scaling == 'density':
            scale = 1.0 / (self.sample_rate * float((taper * taper).sum()))
        elif scaling == 'spectrum':
            scale = 1.0 / float(taper.sum()) ** 2
        else:
            raise ValueError("scaling must be 'density' or 'spectrum', got %r" % (scaling,))
        cdt = _float_dtype(dtype)
        i0, i1 = self._row_range(start, stop)
        if i1 - i0 < nperseg:
            raise ValueError("welch: rows [%d, %d) hold fewer than nperseg = %d rows" % (i0, i1, nperseg))
        cols, squeeze = self._stats_channels(channels)
        f = np.fft.rfftfreq(nperseg, 1.0 / self.sample_rate)
        nb = nperseg // 2 + 1
        n_seg = (i1 - i0 - nperseg) // step + 1
        total = np.zeros((nb, cols.size))
        if cols.size:
            G = hip.welch_group_segments(step)
            n_groups = -(-n_seg // G)

            def group_keys(g0, g1):                                  # the chunks of the rows read by groups [g0, g1)
                return self._chunk_span(i0 + g0 * G * step, i0 + (min(g1 * G, n_seg) - 1) * step + nperseg)

            # calls: whole groups, cut where the compressed bytes of their chunks pass WELCH_CALL_BYTES
            cuts, acc = [0], 0
            for g in range(n_groups):
                keys = group_keys(g, g + 1)
                b = self.chunk_offsets[keys[-1] + 1] - self.chunk_offsets[keys[0]]
                if acc and acc + b > WELCH_CALL_BYTES:
                    cuts.append(g)
                    acc = 0
                acc += b
            cuts.append(n_groups)

            def part(a, b):
                return group_keys(a, b), (i0, a * G, min(b * G, n_seg), nperseg, step, taper, dt, cdt, cols)
            for _, _, (sums,) in self._halo_parts(self.codec.welch, cuts, part):
                for group in sums:                                   # the range: groups in order, float64, from +0
                    total = total + group
        psd = total * scale
        psd[1:-1] *= 2.0
        psd /= n_seg
        return f, (psd[:, 0] if squeeze else psd)

    # -- channel covariance on the device (an extension: the reference's users form x.T @ x of Reader[...] on the host)
    def cov(self, start=0, stop=None, channels=slice(None), window=None, ddof=1, taps=None, reference=None):
        """Per-window channel x channel covariance of rows [start, stop), on the device: only one Gram matrix and one row of sums per
        group of rows cross the bus.  Per window this is np.cov(self[w0:w1, channels], rowvar=False, ddof=ddof) up to rounding.
        Windows are [start + w * window, min(start + (w + 1) * window, stop)); window=None is one window over the range.  start / stop
        follow Reader[...]; channels: an int (C = 1: nothing is squeezed), a slice with step >= 1, or a sequence of ints in any order,
        repeats allowed.  ddof: an int >= 0.  Returns a Bunch: count (n_windows,) int64; sum (n_windows, C): int64 with numpy's wrap
        for integer dtypes, float64 for floats; gram (n_windows, C, C) = sum over rows of x[t, i] * x[t, j]: int64 and exact (numpy's
        wrap included) for 1- and 2-byte integers, else float64 with the items converted to float64 once (8-byte integers rounded);
        mean = sum / count; cov = (float64(gram) - np.outer(float64(sum), mean)) / (count - ddof), NaN where count - ddof <= 0; start,
        stop, window, channels.  The summation tree (include/mtscomp_hip.h, mts_gram) depends on the rows' offsets in their window
        only: the same bits whatever the lanes, calls, cache residency, column set or order; G[i, j] and G[j, i] are equal.
        float64 subnormals are kept, as items and as results: nothing is flushed to zero, and a product below 2^-1022 is rounded to
        a multiple of 2^-1074 like any IEEE product (the error bound in the header has an absolute term n * 2^-1074 for it).  The
        raw-moment formula loses relative accuracy on float data whose mean is large compared with its spread (no centred two-pass
        form).  Chunks resident in the device cache are read where they lie; the others are decoded in a transient workspace and NOT
        kept.  A damaged chunk raises the IOError of Reader[...].
        taps= / reference= (as detect takes them; either given): the rows are z[t, j], the filtered rows of detect -- float32, the
        bytes of decimate(1, taps=taps, edge='recording', dtype=float32) on `channels` (taps=None is [1.0]) minus, with
        reference='median', the float32 median over the selected columns of each row; the bytes of residual([], ...).  z is made
        and reduced on the device slab by slab and never crosses the bus (mts_filtered_gram).  Everything above is then the contract
        for a float32 recording whose items are z: gram and sum are float64, the summation tree is the same.  With the median
        reference the result is NOT independent of the column set (the median is over the selected columns), and a NaN in a row
        poisons every entry of that row's window, not only those of its own column.  The Bunch then also carries taps (the float64
        array used) and reference.  The same bits whatever the lanes, calls, pieces, slabs or cache residency; a damaged chunk in
        the filter's support raises the IOError of Reader[...].  Whitening in the spike band, z never leaving the device:
            hp = highpass_taps(300, r.sample_rate, 101)
            c = r.cov(taps=hp, reference='median')
            W = whitening_weights(c.cov[0], 1e-6)
            white = r.correlate(W.T[:, None, :], before=0, taps=hp, reference='median')     # T = 1 templates: project applied to z
        and a matched filter in whitened space is correlate on z with the whitening folded into the templates on the host,
        K'[k, tau, i] = sum_j W[i, j] * Kw[k, tau, j]."""
        filt = self._rank_filter(taps, reference, channels)
        if filt:
            self._need_codec('cov', 'filtered_gram', 'forms Gram matrices of the filtered rows')
        else:
            self._need_codec('cov', 'gram', 'forms Gram matrices')
        n_taps = int(filt[0].size) if filt else 1
        i0, i1 = self._row_range(start, stop)
        window = _window_rows(window, i0, i1)
        if not isinstance(ddof, (int, np.integer)) or isinstance(ddof, bool) or ddof < 0:
            raise ValueError("ddof must be an int >= 0, got %r" % (ddof,))
        ddof = int(ddof)
        cols, _ = self._stats_channels(channels)
        nc = int(cols.size)
        n_win = -(-(i1 - i0) // window)
        g_dt, s_dt = hip.gram_dtypes(np.float32 if filt else self.dtype)       # (z is float32)
        gram = np.zeros((n_win, nc, nc), g_dt)
        sm = np.zeros((n_win, nc), s_dt)
        cnt = np.minimum(window, i1 - i0 - window * np.arange(n_win, dtype=np.int64)).astype(np.int64)
        if n_win and nc:
            K = -(-window // hip.GRAM_GROUP_ROWS)
            n_groups = hip.gram_groups(i0, i1, window)
            g = np.arange(n_groups, dtype=np.int64)
            w0 = i0 + (g // K) * window
            glo = w0 + (g % K) * hip.GRAM_GROUP_ROWS
            ghi = np.minimum(np.minimum(glo + hip.GRAM_GROUP_ROWS, w0 + window), i1)
            bounds, offsets = np.asarray(self.chunk_bounds, np.int64), np.asarray(self.chunk_offsets, np.int64)
            # the chunks a group reads: those of its rows' filter support (_support; one tap: the rows themselves)
            half = (n_taps - 1) // 2
            gc0 = np.searchsorted(bounds, np.maximum(0, glo + half - (n_taps - 1)), 'right') - 1
            gc1 = np.searchsorted(bounds, np.minimum(self.n_samples, ghi + half) - 1, 'right') - 1
            # calls: whole groups, cut where the compressed bytes of their chunks pass GRAM_CALL_BYTES or their results GRAM_SLAB_BYTES
            cum = np.concatenate(([0], np.cumsum(offsets[gc1 + 1] - offsets[gc0])))
            per_call = max(1, GRAM_SLAB_BYTES // (8 * (nc * nc + nc)))
            cuts = [0]
            while cuts[-1] < n_groups:
                a = cuts[-1]
                b = int(np.searchsorted(cum, cum[a] + GRAM_CALL_BYTES, 'right')) - 1
                cuts.append(min(n_groups, a + per_call, max(b, a + 1)))

            def part(a, b):
                keys = list(range(int(gc0[a]), int(gc1[b - 1]) + 1))
                if filt:
                    return keys, (0, self.n_samples, filt[0], cols, filt[1], i0, i1, window, a, b)
                return keys, (i0, i1, window, a, b, cols)
            fn = self.codec.filtered_gram if filt else self.codec.gram
            for a, b, (gp, sp) in self._halo_parts(fn, cuts, part):      # groups in order: the float sums are the same every time
                if K == 1:
                    gram[a:b] += gp
                    sm[a:b] += sp
                else:
                    for z in range(b - a):
                        gram[(a + z) // K] += gp[z]
                        sm[(a + z) // K] += sp[z]
        with np.errstate(invalid='ignore', divide='ignore'):
            sf = sm.astype(np.float64)
            mean = sf / cnt[:, None]
            denom = cnt - ddof
            cov = (gram.astype(np.float64) - sf[:, :, None] * mean[:, None, :]) / denom[:, None, None]
        cov[denom <= 0] = np.nan
        out = Bunch(count=cnt, sum=sm, gram=gram, mean=mean, cov=cov, start=i0, stop=i1, window=window, channels=cols)
        if filt:
            out.update(taps=filt[0], reference=reference)
        return out

    def _read_range(self, b0, b1):
        """The compressed bytes of chunks b0 .. b1-1 in one read."""
        base = self.chunk_offsets[b0]
        return self._pread(self.chunk_offsets[b1] - base, base)

    def _decode_into(self, b0, b1, dst, buf=None, lane=None):
        """Chunks b0 .. b1-1 (consecutive in the file) decoded straight into `dst` (their rows, C-contiguous): one read (or
        the bytes read ahead by the caller), one codec call (on `lane` of the codec, if given), no copy on the host and
        nothing left in the chunk cache."""
        base = self.chunk_offsets[b0]
        if buf is None:
            buf = self._read_range(b0, b1)
        offs = [self.chunk_offsets[i] - base for i in range(b0, b1)]
        lens = [self.chunk_offsets[i + 1] - self.chunk_offsets[i] for i in range(b0, b1)]
        rows = [self.chunk_bounds[i + 1] - self.chunk_bounds[i] for i in range(b0, b1)]
        extra = {} if lane is None else {'lane': lane}
        status, _ = self.codec.decompress((buf, offs, lens), rows, self.n_channels, self.dtype, self._flags(), out=dst, **extra)
        self._raise_for(dict(zip(range(b0, b1), status)))

    def read_chunk(self, chunk_idx, chunk_start, chunk_length):
        """One decoded chunk, (n_samples_chunk, n_channels), C-contiguous (mtscomp.py:602-635)."""
        return self._decode([(chunk_idx, chunk_start, chunk_length)])[chunk_idx]

    def _decompress_chunk(self, chunk_idx):
        """mtscomp.py:637-643."""
        assert 0 <= chunk_idx <= self.n_chunks - 1
        start = self.chunk_offsets[chunk_idx]
        return chunk_idx, self.read_chunk(chunk_idx, start, self.chunk_offsets[chunk_idx + 1] - start)

    def decompress_chunks(self, chunk_ids, pool=None):
        """{chunk_idx: array} for the requested chunks, decoded in one device batch
        (mtscomp.py:645-650; `pool` is accepted for compatibility and not needed)."""
        ids = list(chunk_ids)
        triples = [(i, self.chunk_offsets[i], self.chunk_offsets[i + 1] - self.chunk_offsets[i]) for i in ids]
        with self._cache_lock:
            keep = self.cache_size
            if len(ids) > keep:
                self.cache_size = len(ids)          # a batch must not evict itself
            try:
                out = self._decode(triples)
            finally:
                self.cache_size = keep
                self._trim_cache()
        assert set(out.keys()) == set(ids)
        return out

    def _validate_index(self, i, value_for_none=0):
        """A slice bound as a sample index in [0, n_samples]: None -> the default, negative -> from the end (mtscomp.py:652-659)."""
        if i is None:
            return int(_clip(value_for_none, 0, self.n_samples))
        return int(_clip(i + self.n_samples if i < 0 else i, 0, self.n_samples))

    def _chunks_for_interval(self, i0, i1):
        """First and last chunk to load for samples [i0, i1] -- i1 is treated as inclusive, exactly
        like the reference (mtscomp.py:661-684; table pinned by tests.py:308-339)."""
        i0 = _clip(i0, 0, self.n_samples - 1)
        i1 = _clip(i1, i0, self.n_samples - 1)
        first = _clip(bisect.bisect_right(self.chunk_bounds, i0) - 1, 0, self.n_chunks - 1)
        last = _clip(bisect.bisect_right(self.chunk_bounds, i1, lo=first) - 1, 0, self.n_chunks - 1)
        assert 0 <= first <= last <= self.n_chunks - 1
        return first, last

    def start_thread_pool(self):
        """Kept for API compatibility (mtscomp.py:686-692); the device path does not need it."""
        if self.pool:  # pragma: no cover
            return self.pool
        self.pool = ThreadPool(max(1, min(4, int(self.config.n_threads or 1))))
        return self.pool

    def stop_thread_pool(self):
        """mtscomp.py:694-699."""
        if self.pool:
            self.pool.close()
            self.pool.join()
        self.pool = None

    def tofile(self, out, overwrite=False, in_place=None):
        """Decompress the whole file to a flat binary file (mtscomp.py:701-743).  With `overwrite` an existing file is unlinked
        first and a NEW file written, as the reference does (mtscomp.py:711-715): hard links to the old file, memory maps of it and
        its owner / mode are left alone.  `in_place=True` (or MTSCOMP_TOFILE_IN_PLACE=1) is an opt-in that is NOT the reference's
        behaviour: an existing regular file is written over where it is (same inode, cut to the new length at the end) -- faster
        on a RAM-backed file system, whose pages are there already; readers of the old file see their data change."""
        if out is None:
            out = Path(self.cdata.name).with_suffix('.bin')
        out = Path(out)
        if not overwrite and out.exists():  # pragma: no cover
            raise ValueError("The output file %s already exists, use --overwrite or specify another "
                             "output path." % out)
        if in_place is None:
            in_place = os.environ.get('MTSCOMP_TOFILE_IN_PLACE', '0') not in ('', '0')
        direct = getattr(self.codec, 'takes_out', False)
        pipelined = direct and self.n_chunks > 1
        keep_inode = bool(in_place) and pipelined and out.is_file() and not out.is_symlink()
        if overwrite and out.exists() and not keep_inode:
            _unlink_lazily(out)
        if pipelined:
            dsize = self._tofile_pipelined(out, keep_inode)
        else:
            with open(out, 'wb') as fb:
                for batch in range(self.n_batches):
                    first = self.batch_size * batch
                    last = min(self.batch_size * (batch + 1), self.n_chunks)
                    chunks = self.decompress_chunks(range(first, last))
                    for idx in sorted(chunks.keys()):
                        fb.write(chunks[idx])
                dsize = fb.tell()
        assert dsize == self.chunk_bounds[-1] * self.n_channels * self.dtype.itemsize
        logger.info("Wrote %s (%.1f GB).", out, dsize / 1024 ** 3)
        if self.check_after_decompress:
            decompressed = load_raw_data(out, n_channels=self.n_channels, dtype=self.dtype)
            check(decompressed, self.cdata, self.cmeta, codec=self._codec)

    def _tofile_pipelined(self, out, keep_inode=False):
        """The file written piece by piece.  Per lane of the codec (a HipCodec has one per device; piece k goes to lane k mod
        lanes) three things are in flight: the compressed bytes of the lane's next piece being read, a piece on the device
        (decoded straight into one of the lane's two host buffers), the piece before being written by a few threads (pwrite on
        disjoint ranges; file writes, reads and ctypes calls all release the GIL).  A piece is a fraction of a device batch so
        that even a one-batch file overlaps its copies with its writes.  The host buffers are page-locked when the codec has
        such memory -- the decoded rows arrive by DMA, without a copy out of a staging piece -- and come from a pool that outlives
        the call (pinning a few hundred MB takes longer than writing them).  Returns the size of the file."""
        lanes = self._n_lanes() if getattr(self.codec, 'takes_out', False) else 1
        piece = max(1, min(self.batch_size, TOFILE_PIECE_CHUNKS))
        starts = list(range(0, self.n_chunks, piece))
        lanes = max(1, min(lanes, len(starts)))
        row_bytes = self.n_channels * self.dtype.itemsize
        max_rows = max(self.chunk_bounds[min(b0 + piece, self.n_chunks)] - self.chunk_bounds[b0] for b0 in starts)
        n_bufs = min(2 * lanes, len(starts))
        take, give = getattr(self.codec, 'host_buffer_take', None), getattr(self.codec, 'host_buffer_give', None)
        max_cbytes = max(self.chunk_offsets[min(b0 + piece, self.n_chunks)] - self.chunk_offsets[b0] for b0 in starts)
        pinned, pinned_in = [], []
        if take is not None and give is not None and hasattr(os, 'preadv'):
            try:
                for _ in range(n_bufs):
                    pinned.append(take(max_rows * row_bytes))
                for _ in range(n_bufs):                             # the compressed bytes of a piece are read into page-locked memory too:
                    pinned_in.append(take(max_cbytes + 64))          # no fresh pages to fault in per piece, and the DMA reads them where they are
            except Exception:  # noqa: BLE001  (no page-locked memory to be had: pageable buffers do)
                for h in pinned + pinned_in:
                    give(h)
                pinned, pinned_in = [], []
        if pinned:
            bufs = [h.array[:max_rows * row_bytes].view(self.dtype).reshape(max_rows, self.n_channels) for h in pinned]
        else:
            bufs = [np.empty((max_rows, self.n_channels), dtype=self.dtype) for _ in range(n_bufs)]
        n_writers = max(1, int(os.environ.get('MTSCOMP_TOFILE_WRITERS', TOFILE_WRITERS)))
        # a new file (the reference's open(out, 'wb') after its unlink) unless tofile(in_place=True) found a file to write over:
        # that one keeps its pages and is cut to the new length when everything is written
        fd = os.open(str(out), os.O_WRONLY | os.O_CREAT | (0 if keep_inode else os.O_TRUNC), 0o644)
        total_bytes = self.chunk_bounds[-1] * row_bytes

        def write_piece(arr, offset):
            mv = memoryview(arr).cast('B')
            per = (len(mv) + n_writers - 1) // n_writers
            per = max(1 << 20, (per + 4095) & ~4095)

            def one(k):
                a, b = k * per, min((k + 1) * per, len(mv))
                while a < b:
                    a += os.pwrite(fd, mv[a:b], offset + a)
            parts = [k for k in range(n_writers) if k * per < len(mv)]
            if len(parts) == 1:
                one(0)
            else:
                wpool.map(one, parts, chunksize=1)

        def piece_range(k):
            return starts[k], min(starts[k] + piece, self.n_chunks)

        def read_piece(k, into):
            """The compressed bytes of piece k: into the page-locked buffer `into` (-> a view of it, 16 spare bytes behind the last
            chunk zeroed: the kernels may read a few bytes past a stream), or as a bytes object."""
            b0, b1 = piece_range(k)
            if into is None:
                return self._read_range(b0, b1)
            base, n = self.chunk_offsets[b0], self.chunk_offsets[b1] - self.chunk_offsets[b0]
            mv, a = memoryview(into.array), 0
            while a < n:
                got = os.preadv(self.cdata.fileno(), [mv[a:n]], base + a)
                if got <= 0:
                    break
                a += got
            assert a == n
            into.array[n:n + 16] = 0
            return into.array[:n + 16]

        def lane_loop(g):
            mine = list(range(g, len(starts), lanes))            # this lane's pieces
            my_bufs = bufs[g::lanes]
            my_in = pinned_in[g::lanes] or [None]                   # (the read ahead fills the one the device is not reading)
            aux = ThreadPool(2)                                     # (one thread reads ahead, one hands pieces to the writers)
            try:
                nxt = aux.apply_async(read_piece, (mine[0], my_in[0]))
                pending = [None] * len(my_bufs)
                for j, k in enumerate(mine):
                    b0, b1 = piece_range(k)
                    buf = nxt.get()
                    nxt = aux.apply_async(read_piece, (mine[j + 1], my_in[(j + 1) % len(my_in)])) if j + 1 < len(mine) else None
                    slot = j % len(my_bufs)
                    if pending[slot] is not None:
                        pending[slot].get()                         # (the write that used this buffer two pieces ago)
                    rows = self.chunk_bounds[b1] - self.chunk_bounds[b0]
                    dst = my_bufs[slot][:rows]
                    self._decode_into(b0, b1, dst, buf, lane=g if lanes > 1 else None)
                    pending[slot] = aux.apply_async(write_piece, (dst, self.chunk_bounds[b0] * row_bytes))
                for p in pending:
                    if p is not None:
                        p.get()
            finally:
                # also on the way out of a failure (a corrupt chunk raises in _decode_into): a read or a write still in flight is
                # waited for -- ThreadPool's context manager terminate()s without joining, and the caller is about to truncate and
                # close the descriptor and hand the page-locked buffers back to the pool
                aux.close()
                aux.join()

        wpool = ThreadPool(n_writers)
        try:
            try:
                if lanes == 1:
                    lane_loop(0)
                else:
                    self.codec.run_lanes(lane_loop, lanes)
            finally:
                wpool.close()                                       # (every lane has joined its own helpers by now: nothing writes any more)
                wpool.join()
            if os.fstat(fd).st_size > total_bytes:
                os.ftruncate(fd, total_bytes)                       # (what a longer file of that name had behind)
            return os.fstat(fd).st_size
        except BaseException:
            try:
                os.ftruncate(fd, 0)                                 # (a failed write leaves no mixture of the old file and the new)
            except OSError:
                pass
            raise
        finally:
            os.close(fd)
            del bufs
            for h in pinned + pinned_in:
                give(h)

    def close(self):
        """mtscomp.py:745-748."""
        with self._dev_cache_lock:
            caches, self._dev_caches = self._dev_caches or [], None
        for cache in caches:
            if cache is not None:
                try:
                    self.codec.cache_destroy(cache)
                except Exception:  # pragma: no cover
                    pass
        with self._map_lock:
            self._cmap_view = None
            if self._cmap is not None:
                try:
                    self._cmap.close()
                except (BufferError, ValueError):                  # (a view is still out somewhere: the mapping goes with it)
                    pass
                self._cmap = None
        with self._pin_lock:                                      # (a slice on another thread may be reading into the buffer)
            if self._io_pool is not None:
                self._io_pool.close()
                self._io_pool = None
            if self._pin is not None:
                pin, self._pin = self._pin, None
                give = getattr(self.codec, 'host_buffer_give', None)
                (give or (lambda h: h.free()))(pin)
        if self.cdata:
            self.cdata.close()

    def chop(self, n_chunks, out=None):
        """Write the first n_chunks chunks as a new .cbin/.ch pair without decoding anything: the byte range up to
        chunk_offsets[n_chunks], a header cut to match, sha1s dropped and 'chopped' set (mtscomp.py:750-796)."""
        assert n_chunks > 0
        if n_chunks >= self.n_chunks:  # pragma: no cover
            logger.warning("Cannot chop more chunks than there are in the original file.")
            return
        assert out is not None, "The output path must be specified."
        out = Path(out)
        outmeta = out.with_suffix('.ch')
        assert out.suffix == '.cbin'
        for target in (out, outmeta):
            if target.exists():  # pragma: no cover
                raise IOError("File %s already exists." % target)
        out.parent.mkdir(parents=True, exist_ok=True)
        n_bytes = self.chunk_offsets[n_chunks]
        out.write_bytes(self._pread(n_bytes, 0))
        header = dict(self.cmeta)
        header.update(chunk_bounds=self.cmeta['chunk_bounds'][:n_chunks + 1], chunk_offsets=self.cmeta['chunk_offsets'][:n_chunks + 1],
                      sha1_compressed=None, sha1_uncompressed=None, chopped=True)
        assert header['chunk_offsets'][-1] == n_bytes
        outmeta.write_text(json.dumps(header, indent=2, sort_keys=True))

    def __getitem__(self, item):
        """NumPy-style slicing (mtscomp.py:798-856).  All chunks a slice touches are decoded in one
        device batch."""
        fallback = np.zeros((0, self.n_channels), dtype=self.dtype)
        if isinstance(item, slice):
            i0 = self._validate_index(item.start, 0)
            i1 = self._validate_index(item.stop, self.n_samples)
            if i1 <= i0:
                return fallback
            first, last = self._chunks_for_interval(i0, i1)
            # the reference also loads the chunk that starts exactly at i1 (inclusive stop); its rows
            # are never part of the result, so it is not decoded here
            if last > first and self.chunk_bounds[last] >= i1:
                last -= 1
            rows = self._slice_from_device_cache(first, last, i0, i1)
            if rows is not None:
                out = rows[0:i1 - i0:item.step, :]             # (like arr[a:b:step] in the reference: a negative step gives nothing)
                assert out.shape[0] == len(range(i0, i1, item.step or 1))
                return out
            if last - first + 1 > self.batch_size:
                # a long slice: batch after batch straight into the result (one codec call for everything would need the
                # whole slice in device memory, and the chunk cache could not hold it anyway)
                r0 = self.chunk_bounds[first]
                whole = np.empty((self.chunk_bounds[last + 1] - r0, self.n_channels), dtype=self.dtype)   # whole chunks first..last
                direct = getattr(self.codec, 'takes_out', False)
                per_call = max(1, self.batch_chunks) if direct else self.batch_size      # (direct: a call is one lane's, i.e. one device's)
                starts = list(range(first, last + 1, per_call))
                lanes = max(1, min(self._n_lanes(), len(starts))) if direct else 1

                def lane_loop(g):
                    mine = starts[g::lanes]
                    ahead = ThreadPool(1) if direct and len(mine) > 1 else None      # the next batch's bytes are read while this one is on the device
                    nxt = ahead.apply_async(self._read_range, (mine[0], min(mine[0] + per_call, last + 1))) if ahead else None
                    for k, b0 in enumerate(mine):
                        b1 = min(b0 + per_call, last + 1)
                        dst = whole[self.chunk_bounds[b0] - r0:self.chunk_bounds[b1] - r0]
                        if direct:
                            buf = nxt.get() if nxt is not None else None
                            nxt = ahead.apply_async(self._read_range, (mine[k + 1], min(mine[k + 1] + per_call, last + 1))) \
                                if ahead and k + 1 < len(mine) else None
                            self._decode_into(b0, b1, dst, buf, lane=g if lanes > 1 else None)
                        else:
                            chunks = self.decompress_chunks(range(b0, b1))
                            for idx in range(b0, b1):
                                dst[self.chunk_bounds[idx] - self.chunk_bounds[b0]:self.chunk_bounds[idx + 1] - self.chunk_bounds[b0]] = chunks[idx]
                            del chunks
                    if ahead:
                        ahead.close()
                if lanes == 1:
                    lane_loop(0)
                else:
                    self.codec.run_lanes(lane_loop, lanes)
                out = whole[i0 - r0:i1 - r0:item.step, :]
                assert out.shape[0] == len(range(i0, i1, item.step or 1))
                return out
            triples = list(self.iter_chunks(first, last))
            with self._cache_lock:
                keep = self.cache_size
                if len(triples) > keep:
                    self.cache_size = len(triples)
                try:
                    decoded = self._decode(triples)
                finally:
                    self.cache_size = keep
                    self._trim_cache()
            chunks = [decoded[i] for i in range(first, last + 1)]
            arr = _join_rows(chunks)
            a = i0 - self.chunk_bounds[first]
            b = i1 - self.chunk_bounds[first]
            assert 0 <= a <= b <= arr.shape[0]
            out = arr[a:b:item.step, :]
            assert out.shape[0] == len(range(i0, i1, item.step or 1))
            return out
        elif isinstance(item, tuple):
            if len(item) == 1:
                return self[item[0]]
            elif len(item) == 2 and np.isscalar(item[0]):
                return self[item[0]][item[1]]
            elif len(item) == 2:
                got = self.read_slices([item], _fallback=False)
                if got is not None:
                    return got[0]
                return self[item[0]][:, item[1]]
        elif isinstance(item, (int, np.integer)):
            item = int(item)
            if item < 0:
                item += self.n_samples * (-(item // self.n_samples))
                assert 0 <= item < self.n_samples
            if not 0 <= item < self.n_samples:  # pragma: no cover
                raise IndexError("index %d is out of bounds for axis 0 with size %d" % (item, self.n_samples))
            return self[item:item + 1][0]
        elif isinstance(item, (list, np.ndarray)):  # pragma: no cover
            raise NotImplementedError("Indexing with multiple values is currently unsupported.")
        return fallback  # pragma: no cover

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass


# ------------------------------------------------------------------------------------------------
# high-level API (mtscomp.py:862-997)
# ------------------------------------------------------------------------------------------------
def check(data, out, outmeta, codec=None):
    """Decompress everything and compare with `data` (mtscomp.py:866-888)."""
    unc = decompress(out, outmeta, codec=codec)
    try:
        for first in range(0, unc.n_chunks, unc.batch_size):
            ids = range(first, min(first + unc.batch_size, unc.n_chunks))
            chunks = unc.decompress_chunks(ids)
            for idx in ids:
                chunk = chunks[idx]
                expected = data[unc.chunk_bounds[idx]:unc.chunk_bounds[idx + 1]]
                assert chunk.dtype == expected.dtype
                assert chunk.shape == expected.shape
                if np.issubdtype(chunk.dtype, np.integer):
                    assert np.array_equal(chunk, expected)
                else:
                    assert np.allclose(chunk, expected, atol=CHECK_ATOL)
    finally:
        unc.close()


def compress(path, out=None, outmeta=None, sample_rate=None, n_channels=None, dtype=None, codec=None, **kwargs):
    """Compress a flat binary (or .npy) file into `out` (.cbin) + `outmeta` (.ch); returns the
    compression ratio, as the reference does (mtscomp.py:891-958)."""
    w = Writer(codec=codec, **kwargs)
    w.open(path, sample_rate=sample_rate, n_channels=n_channels, dtype=dtype)
    ratio = w.write(out, outmeta)
    w.close()
    return ratio


def decompress(cdata, cmeta=None, out=None, write_output=False, overwrite=False, codec=None, **kwargs):
    """Open a compressed dataset; optionally write it out decompressed (mtscomp.py:961-997)."""
    if out:
        write_output = True
    r = Reader(codec=codec, **kwargs)
    r.open(cdata, cmeta)
    if write_output:
        r.tofile(out, overwrite=overwrite)
    return r
