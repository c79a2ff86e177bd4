"""ctypes binding of libmtscomp_hip.so (include/mtscomp_hip.h).

This is the only compute path of the package: there is no CPU fallback.  Loading fails loudly when
the shared library has not been built (``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C mtscomp_amd/csrc``) and every compute call raises ``HipError`` when no MI355X is visible.
"""
import ctypes as C
import math
import os
import warnings
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent

# (MTSCOMP_HIP_LIB: another build of the same library, for A/B measurements -- tools/ab_stage_times.py; said out loud when used)
LIB_PATH = Path(os.environ.get('MTSCOMP_HIP_LIB') or _HERE / 'libmtscomp_hip.so')
if os.environ.get('MTSCOMP_HIP_LIB'):
    warnings.warn('mtscomp_amd: MTSCOMP_HIP_LIB replaces the in-tree library with %s' % LIB_PATH, RuntimeWarning, stacklevel=2)

FLAG_TIME_DIFF = 1
FLAG_SPATIAL_DIFF = 2
FLAG_ORDER_F = 4
FLAG_FLOAT = 8
FLAG_UNSIGNED = 16          # integer items are unsigned (window statistics only)

CHUNK_OK = 0
CHUNK_CORRUPT = -1
CHUNK_BADSIZE = -2

E_NODEV = -2
E_UNSUPPORTED = -5
E_MISS = -7


class HipError(RuntimeError):
    def __init__(self, code, what, detail=''):
        self.code = code
        super().__init__('%s failed: %s (%d)%s' % (what, _strerror(code), code, (': ' + detail) if detail else ''))


_lib = None


def _strerror(code):
    try:
        return lib().mts_strerror(code).decode()
    except Exception:  # pragma: no cover
        return '?'


def lib():
    """The loaded shared library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            '%s is missing: build the HIP extension first (make -C mtscomp_amd/csrc). '
            'mtscomp_amd has no CPU code path.' % LIB_PATH)
    L = C.CDLL(str(LIB_PATH))
    vp, lp, ip = C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_int)
    L.mts_version.restype = C.c_int
    L.mts_device_count.restype = C.c_int
    L.mts_strerror.restype = C.c_char_p
    L.mts_strerror.argtypes = [C.c_int]
    L.mts_last_error.restype = C.c_char_p
    L.mts_compress_bound.restype = C.c_long
    L.mts_compress_bound.argtypes = [C.c_long]
    L.mts_delta_transpose.argtypes = [C.c_int, vp, C.c_long, C.c_int, C.c_int, C.c_int, vp]
    L.mts_cumsum_transpose.argtypes = [C.c_int, vp, C.c_long, C.c_int, C.c_int, C.c_int, vp]
    L.mts_compress_chunks.argtypes = [C.c_int, vp, C.c_int, C.c_int, lp, C.c_int, C.c_int, C.c_int, vp, lp, lp]
    L.mts_decompress_chunks.argtypes = [C.c_int, vp, lp, lp, lp, C.c_int, C.c_int, C.c_int, C.c_int, vp, lp, ip]
    L.mts_dev_compress_chunks.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, lp, C.c_int, C.c_int, C.c_int, vp, lp, lp]
    L.mts_dev_decompress_chunks.argtypes = [C.c_int, vp, vp, lp, lp, lp, C.c_int, C.c_int, C.c_int, C.c_int, vp, lp, ip]
    L.mts_dev_synth_int16.argtypes = [C.c_int, vp, vp, C.c_long, C.c_long, C.c_int, C.c_long]
    L.mts_host_alloc.argtypes = [C.c_long, C.POINTER(vp)]
    L.mts_host_free.argtypes = [vp]
    L.mts_dev_alloc.argtypes = [C.c_int, C.c_long, C.POINTER(vp)]
    L.mts_dev_free.argtypes = [C.c_int, vp]
    L.mts_dev_copy.argtypes = [C.c_int, vp, vp, vp, C.c_long, C.c_int]
    L.mts_dev_sync.argtypes = [C.c_int]
    L.mts_dev_compare.argtypes = [C.c_int, vp, vp, vp, C.c_long, lp, lp]
    L.mts_last_stage_times.restype = C.c_int
    L.mts_last_stage_times.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    L.mts_debug_match_tables.argtypes = [C.c_int, vp, C.c_long, C.c_int, vp, vp]
    L.mts_debug_tokens.argtypes = [C.c_int, vp, C.c_long, C.c_int, vp, lp]
    L.mts_debug_deflate.argtypes = [C.c_int, vp, C.c_long, C.c_int, vp, C.c_long, lp]
    L.mts_debug_inflate.argtypes = [C.c_int, vp, C.c_long, vp, C.c_long, lp, ip]
    L.mts_cache_create.argtypes = [C.c_int, C.c_long, lp]
    L.mts_cache_destroy.argtypes = [C.c_long]
    L.mts_cache_query.argtypes = [C.c_long, lp, C.c_int, ip]
    L.mts_cache_read_rows.argtypes = [C.c_long, C.c_int, lp, vp, lp, lp, lp, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long,
                                      vp, ip]
    L.mts_cache_read_slices.argtypes = [C.c_long, C.c_int, lp, vp, lp, lp, lp, C.c_int, C.c_int, C.c_int, C.c_int, lp, vp, lp,
                                        C.c_long, ip]
    L.mts_cache_read_slices_leading.argtypes = [C.c_long, C.c_int, lp, vp, lp, lp, lp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, lp, vp, lp,
                                                C.c_long, ip]
    # the device reductions: the chunk table (host entry: device, cache, n, keys, row0, cdata, offs, lens, rows, n_channels, itemsize,
    # flags; device entry: device, stream, cbuf, offs, lens, row0, rows, n, n_channels, itemsize, flags), the op's own arguments, the
    # results and the status
    host = [C.c_int, C.c_long, C.c_int, lp, lp, vp, lp, lp, lp, C.c_int, C.c_int, C.c_int]
    dev = [C.c_int, vp, vp, lp, lp, lp, lp, C.c_int, C.c_int, C.c_int, C.c_int]
    ci, cl, dp, fp, up = C.c_int, C.c_long, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)
    for name, mid, tail, dev_tail in (
            ('window_stats', [cl, cl, cl, ci, ip], [vp, vp, vp, vp, lp, ip], None),
            ('decimate', [cl, cl, cl, cl, ci, ci, dp, ci, ci, ip], [vp, ip], None),
            ('project', [cl, cl, ci, ip, dp, ci, dp, ci], [vp, ip], None),
            ('detect', [cl, cl, cl, cl, ci, dp, ci, ip, fp, ci, ci, ci, ci, cl], [vp, vp, vp, lp, ip], None),
            ('waveforms', [cl, cl, ci, dp, ci, ip, ci, cl, lp, ip, ci, ci, ci], [vp, vp, vp, vp, vp, ip], None),
            ('mean_waveforms', [cl, cl, ci, dp, ci, ip, ci, cl, lp, ip, ip, ci, ci, ci, ci, C.c_double], [vp, vp, vp, ip], None),
            ('waveform_features', [cl, cl, ci, dp, ci, ip, ci, cl, lp, ip, ci, ci, ci, ci, fp], [vp, ip], None),
            ('localize', [cl, cl, ci, dp, ci, ip, ci, cl, lp, ip, ci, ci, ci, ci, ci, fp], [vp, vp, vp, vp, ip], None),
            ('correlate', [cl, cl, cl, cl, ci, dp, ci, ip, ci, ci, ci, ci, fp], [vp, ip], None),
            ('match_templates', [cl, cl, cl, cl, ci, dp, ci, ip, ci, ci, ci, ci, fp, fp, ci, cl], [vp, vp, vp, lp, ip], None),
            ('residual', [cl, cl, cl, cl, ci, dp, ci, ip, ci, ci, ci, ci, fp, cl, lp, ip, fp], [vp, ip], None),
            ('match_residual', [cl, cl, cl, cl, ci, dp, ci, ip, ci, ci, ci, ci, fp, fp, ci, cl, cl, lp, ip, fp], [vp, vp, vp, lp, ip], None),
            ('welch', [cl, cl, cl, ci, cl, dp, ci, ci, ci, ip], [vp, ip], None),
            ('gram', [cl, cl, cl, cl, cl, ci, ip], [vp, vp, ip], None),
            ('filtered_gram', [cl, cl, ci, dp, ci, ip, ci, cl, cl, cl, cl, cl], [dp, dp, ip], [vp, vp, ip]),
            ('rank_hist', [cl, cl, cl, ci, ip, ci, dp, up, ip], [C.POINTER(C.c_uint), up, up, lp, ip], [vp, vp, vp, lp, ip]),
            ('filtered_rank_hist', [cl, cl, ci, dp, ci, ip, ci, cl, cl, cl, cl, cl, ci, dp, up, ip], [C.POINTER(C.c_uint), up, up, lp, ip],
             [vp, vp, vp, lp, ip])):
        getattr(L, 'mts_' + name).argtypes = host + mid + tail
        getattr(L, 'mts_dev_' + name).argtypes = dev + mid + (dev_tail or tail)
    L.mts_waveforms_last_plan.argtypes = [C.c_int, lp]
    L.mts_release.restype = None
    _lib = L
    return L


EXPORTS = ['mts_version', 'mts_device_count', 'mts_strerror', 'mts_last_error', 'mts_compress_bound',
           'mts_delta_transpose', 'mts_cumsum_transpose', 'mts_compress_chunks', 'mts_decompress_chunks',
           'mts_dev_compress_chunks', 'mts_dev_decompress_chunks', 'mts_dev_synth_int16',
           'mts_host_alloc', 'mts_host_free', 'mts_dev_alloc', 'mts_dev_free', 'mts_dev_copy', 'mts_dev_sync', 'mts_dev_compare',
           'mts_last_stage_times', 'mts_debug_match_tables', 'mts_debug_tokens', 'mts_debug_deflate',
           'mts_debug_inflate', 'mts_release', 'mts_cache_create', 'mts_cache_destroy', 'mts_cache_query',
           'mts_cache_read_rows', 'mts_cache_read_slices', 'mts_cache_read_slices_leading',
           'mts_window_stats', 'mts_dev_window_stats', 'mts_decimate', 'mts_dev_decimate', 'mts_project', 'mts_dev_project', 'mts_detect', 'mts_dev_detect', 'mts_welch', 'mts_dev_welch',
           'mts_waveforms', 'mts_dev_waveforms', 'mts_waveforms_last_plan', 'mts_mean_waveforms', 'mts_dev_mean_waveforms',
           'mts_waveform_features', 'mts_dev_waveform_features', 'mts_localize', 'mts_dev_localize', 'mts_correlate', 'mts_dev_correlate',
           'mts_match_templates', 'mts_dev_match_templates',
           'mts_residual', 'mts_dev_residual', 'mts_match_residual', 'mts_dev_match_residual',
           'mts_gram', 'mts_dev_gram', 'mts_rank_hist', 'mts_dev_rank_hist', 'mts_filtered_rank_hist', 'mts_dev_filtered_rank_hist',
           'mts_filtered_gram', 'mts_dev_filtered_gram']


def _check(rc, what):
    if rc != 0:
        raise HipError(rc, what, lib().mts_last_error().decode())


def device_count():
    return int(lib().mts_device_count())


def require_device():
    n = device_count()
    if n <= 0:
        raise HipError(E_NODEV, 'mtscomp_amd', 'no MI355X (gfx950) device visible; there is no CPU fallback')
    return n


def compress_bound(n):
    return int(lib().mts_compress_bound(int(n)))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _longs(seq):
    return np.ascontiguousarray(np.asarray(seq, dtype=np.int64))


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_long))


def make_flags(do_time_diff=True, do_spatial_diff=False, chunk_order='F'):
    return ((FLAG_TIME_DIFF if do_time_diff else 0) | (FLAG_SPATIAL_DIFF if do_spatial_diff else 0) |
            (FLAG_ORDER_F if chunk_order == 'F' else 0))


def check_dtype(dtype):
    dtype = np.dtype(dtype)
    if not ((dtype.kind in 'iu' and dtype.itemsize in (1, 2, 4, 8)) or (dtype.kind == 'f' and dtype.itemsize in (4, 8))):
        raise NotImplementedError(
            'the MI355X codec handles integer dtypes of 1/2/4/8 bytes and float32/float64; got %s' % dtype)
    return dtype


def _dflags(flags, dtype):
    """flags as the C ABI wants them: the float bit comes from the dtype."""
    return (int(flags) & ~FLAG_FLOAT) | (FLAG_FLOAT if np.dtype(dtype).kind == 'f' else 0)


# ------------------------------------------------------------------------------------------------
# host-buffer entry points
# ------------------------------------------------------------------------------------------------
def delta_transpose(chunk, flags, device=0):
    chunk = np.ascontiguousarray(chunk)
    check_dtype(chunk.dtype)
    nt, nc = chunk.shape
    out = np.empty(chunk.nbytes, dtype=np.uint8)
    _check(lib().mts_delta_transpose(device, _ptr(chunk), nt, nc, chunk.itemsize, _dflags(flags, chunk.dtype), _ptr(out)),
           'mts_delta_transpose')
    return out


def cumsum_transpose(stream, nt, nc, dtype, flags, device=0):
    dtype = check_dtype(dtype)
    stream = np.ascontiguousarray(np.frombuffer(stream, dtype=np.uint8) if not isinstance(stream, np.ndarray)
                                  else stream.view(np.uint8).ravel())
    assert stream.size == nt * nc * dtype.itemsize
    out = np.empty((nt, nc), dtype=dtype)
    _check(lib().mts_cumsum_transpose(device, _ptr(stream), nt, nc, dtype.itemsize, _dflags(flags, dtype), _ptr(out)),
           'mts_cumsum_transpose')
    return out


def compress_chunks(data, chunk_bounds, flags, level=6, device=0):
    """data: C-contiguous (rows, n_channels) array whose row 0 is chunk_bounds[0].
    Returns the list of zlib streams, one per chunk."""
    data = np.ascontiguousarray(data)
    check_dtype(data.dtype)
    b = _longs(chunk_bounds)
    n_chunks = len(b) - 1
    assert data.shape[0] == b[-1] - b[0]
    row = data.shape[1] * data.itemsize
    bounds = [(compress_bound(int(b[i + 1] - b[i]) * row) + 15) // 16 * 16 for i in range(n_chunks)]
    slots = _longs(np.concatenate(([0], np.cumsum(bounds)))[:-1]) if n_chunks else _longs([])
    out = np.empty(int(sum(bounds)) + 16, dtype=np.uint8)
    sizes = np.zeros(max(n_chunks, 1), dtype=np.int64)
    _check(lib().mts_compress_chunks(device, _ptr(data), data.shape[1], data.itemsize, _lp(b), n_chunks,
                                     _dflags(flags, data.dtype), level, _ptr(out), _lp(slots), _lp(sizes)), 'mts_compress_chunks')
    return [out[int(slots[i]):int(slots[i]) + int(sizes[i])].tobytes() for i in range(n_chunks)]


def decompress_chunks(cbufs, n_rows, n_channels, dtype, flags, device=0, out=None):
    """cbufs: list of bytes-like compressed chunks, or (buffer, offsets, lengths) for chunks that already sit in
    one buffer.  Returns (status list, list of arrays or None).  The arrays are views of ONE output buffer, back to
    back in the order given, so consecutive chunks can be joined without copying.  `out`: a C-contiguous array of
    exactly the decoded size to decode into (the views are then views of it)."""
    dtype = check_dtype(dtype)
    if isinstance(cbufs, tuple):
        buf, offs, lens = cbufs
        n = len(lens)
        if n == 0:
            return [], []
        cdata = np.frombuffer(buf, dtype=np.uint8)
        offs, lens = _longs(offs), _longs(lens)
        if int(offs[-1] + lens[-1]) + 16 > cdata.size:          # the kernels may read a few bytes past a stream
            cdata = np.concatenate((cdata, np.zeros(16, dtype=np.uint8)))
    else:
        n = len(cbufs)
        if n == 0:
            return [], []
        lens = _longs([len(c) for c in cbufs])
        offs = _longs(np.concatenate(([0], np.cumsum(lens)))[:-1])
        cdata = np.frombuffer(b''.join(bytes(c) for c in cbufs) + b'\0' * 16, dtype=np.uint8)
    rows = _longs(n_rows)
    sizes = rows * (n_channels * dtype.itemsize)
    ooffs = _longs(np.concatenate(([0], np.cumsum(sizes)))[:-1])
    if out is None:
        out = np.empty(int(ooffs[-1] + sizes[-1]) + 256, dtype=np.uint8)
    else:
        assert out.flags.c_contiguous and out.nbytes == int(ooffs[-1] + sizes[-1])
        out = out.reshape(-1).view(np.uint8)
    status = np.zeros(n, dtype=np.int32)
    _check(lib().mts_decompress_chunks(device, _ptr(cdata), _lp(offs), _lp(lens), _lp(rows), n, n_channels,
                                       dtype.itemsize, _dflags(flags, dtype), _ptr(out), _lp(ooffs),
                                       status.ctypes.data_as(C.POINTER(C.c_int))), 'mts_decompress_chunks')
    arrays = []
    for i in range(n):
        if status[i] == CHUNK_OK:
            arrays.append(out[int(ooffs[i]):int(ooffs[i] + sizes[i])].view(dtype).reshape(int(rows[i]), n_channels))
        else:
            arrays.append(None)
    return [int(s) for s in status], arrays


# ------------------------------------------------------------------------------------------------
# decoded-chunk cache on the device (Reader random access)
# ------------------------------------------------------------------------------------------------
def cache_create(capacity_bytes, device=0):
    cid = C.c_long(0)
    _check(lib().mts_cache_create(device, int(capacity_bytes), C.byref(cid)), 'mts_cache_create')
    return int(cid.value)


def cache_destroy(cache_id):
    if _lib is not None:
        _lib.mts_cache_destroy(int(cache_id))


def cache_query(cache_id, keys):
    """Per key: 0 = not resident, else the number of channels the resident entry holds."""
    keys = _longs(keys)
    present = np.zeros(keys.size, dtype=np.int32)
    _check(lib().mts_cache_query(int(cache_id), _lp(keys), int(keys.size), present.ctypes.data_as(C.POINTER(C.c_int))),
           'mts_cache_query')
    return present


def cache_read_rows(cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags, row_begin, row_end, out=None):
    """Rows [row_begin, row_end) of the concatenation of the chunks `keys` (file order).  Chunks with lens[i] == 0 must be
    resident (HipError with code E_MISS otherwise).  Returns (status list, (row_end - row_begin, n_channels) array); `out`: a
    C-contiguous array of exactly that shape to fill instead of a new one."""
    dtype = check_dtype(dtype)
    keys, offs, lens, rows = _longs(keys), _longs(offs), _longs(lens), _longs(n_rows)
    n = int(keys.size)
    cdata = np.frombuffer(cdata, dtype=np.uint8) if len(cdata) else np.zeros(16, dtype=np.uint8)
    if n and int((offs + lens).max()) + 16 > cdata.size:          # the kernels may read a few bytes past a stream
        cdata = np.concatenate((cdata, np.zeros(16, dtype=np.uint8)))
    if out is None:
        out = np.empty((int(row_end - row_begin), n_channels), dtype=dtype)
    else:
        assert out.flags.c_contiguous and out.dtype == dtype and out.shape == (int(row_end - row_begin), n_channels)
    status = np.zeros(n, dtype=np.int32)
    _check(lib().mts_cache_read_rows(int(cache_id), n, _lp(keys), _ptr(cdata), _lp(offs), _lp(lens), _lp(rows), n_channels,
                                     dtype.itemsize, _dflags(flags, dtype), int(row_begin), int(row_end), _ptr(out),
                                     status.ctypes.data_as(C.POINTER(C.c_int))), 'mts_cache_read_rows')
    return [int(x) for x in status], out


def cache_read_slices(cache_id, keys, cdata, offs, lens, n_rows, n_channels, dtype, flags, requests, n_leading=None):
    """Several rectangles of the concatenation of the chunks `keys` in one call: requests = [(row_begin, row_end, row_step,
    col_begin, col_end, col_step), ...] (steps >= 1).  The pieces are gathered on the device and come back in one copy.
    Returns (status list, list of 2-D arrays).  n_leading: the requests only touch channels below it, chunks that are not
    resident are decoded up to there only and `lens` may be prefixes of their bytes (mts_cache_read_slices_leading)."""
    dtype = check_dtype(dtype)
    keys, offs, lens, rows = _longs(keys), _longs(offs), _longs(lens), _longs(n_rows)
    n = int(keys.size)
    cdata = np.frombuffer(cdata, dtype=np.uint8) if len(cdata) else np.zeros(16, dtype=np.uint8)
    if n and int((offs + lens).max()) + 16 > cdata.size:          # the kernels may read a few bytes past a stream
        cdata = np.concatenate((cdata, np.zeros(16, dtype=np.uint8)))
    req = _longs(np.asarray(requests, dtype=np.int64).reshape(-1, 6))
    shapes = [(int(-(-(q[1] - q[0]) // q[2])), int(-(-(q[4] - q[3]) // q[5]))) for q in req.reshape(-1, 6)]
    sizes = [(a * b * dtype.itemsize + 255) // 256 * 256 for a, b in shapes]
    out_offs = _longs(np.concatenate(([0], np.cumsum(sizes)))[:-1]) if shapes else _longs([])
    out = np.empty(int(sum(sizes)) + 8, dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.int32)
    _check(lib().mts_cache_read_slices_leading(int(cache_id), n, _lp(keys), _ptr(cdata), _lp(offs), _lp(lens), _lp(rows), n_channels,
                                               dtype.itemsize, _dflags(flags, dtype), int(n_leading or n_channels), len(shapes), _lp(req),
                                               _ptr(out), _lp(out_offs), int(sum(sizes)), status.ctypes.data_as(C.POINTER(C.c_int))),
           'mts_cache_read_slices_leading')
    arrays = [out[int(o):int(o) + a * b * dtype.itemsize].view(dtype).reshape(a, b) for o, (a, b) in zip(out_offs, shapes)]
    return [int(x) for x in status[:n]], arrays


# ------------------------------------------------------------------------------------------------
# the device reductions (extensions: the reference has no such calls).  Every op has a host entry mts_<op> (compressed bytes in host
# memory, resident chunks in a decoded-chunk cache) and a device entry mts_dev_<op> (a DevBuffer of compressed chunks).  Both take the
# chunk table, then the op's own arguments, then the results and the chunks' status: each of the three is marshalled in one place.
# ------------------------------------------------------------------------------------------------
def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ullp(a):
    return a.ctypes.data_as(C.POINTER(C.c_ulonglong))


def _cols32(cols):
    return np.ascontiguousarray(np.asarray(cols, dtype=np.int32))


def stats_flags(flags, dtype):
    """flags as the reductions want them: the float bit and the unsigned bit come from the dtype."""
    return _dflags(flags, dtype) | (FLAG_UNSIGNED if np.dtype(dtype).kind == 'u' else 0)


def _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags):
    """The chunk table of a host entry: chunks `keys` (file rows [row0[i], row0[i] + n_rows[i])), their bytes at offs / lens of cdata.
    cache_id 0: no cache, every chunk comes with its bytes; else chunks with lens[i] == 0 must be resident (HipError E_MISS).
    -> (the leading arguments of mts_<op>, n, the status array to pass last)."""
    dtype = check_dtype(dtype)
    keys, row0, offs, lens, rows = _longs(keys), _longs(row0), _longs(offs), _longs(lens), _longs(n_rows)
    n = int(rows.size)
    cdata = np.frombuffer(cdata, dtype=np.uint8) if len(cdata) else np.zeros(16, dtype=np.uint8)
    assert not n or int((offs + lens).max()) <= cdata.size        # (only the chunks' own bytes are copied: no padding needed here)
    head = (int(device), int(cache_id), n, _lp(keys), _lp(row0), _ptr(cdata), _lp(offs), _lp(lens), _lp(rows), int(n_channels),
            dtype.itemsize, stats_flags(flags, dtype))
    return head, n, np.zeros(max(n, 1), dtype=np.int32)


def _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags):
    """The chunk table of a device entry: compressed chunks at offs / lens of the DevBuffer cbuf.  -> as _host_chunks, for
    mts_dev_<op>."""
    dtype = check_dtype(dtype)
    offs, lens, row0, rows = _longs(offs), _longs(lens), _longs(row0), _longs(n_rows)
    n = int(rows.size)
    head = (cbuf.device, None, cbuf.at(), _lp(offs), _lp(lens), _lp(row0), _lp(rows), n, int(n_channels), dtype.itemsize,
            stats_flags(flags, dtype))
    return head, n, np.zeros(max(n, 1), dtype=np.int32)


def _status(status, n):
    return [int(x) for x in status[:n]]


def _dev_results(out, device, sizes):
    """Room for result arrays of `sizes` bytes in the DevBuffer `out`, each at a 256-byte aligned offset, 256 spare bytes behind
    the last: `out` is made when None or too small.  -> (out, the pointers to hand to the library, the offsets)."""
    at = [0]
    for b in sizes[:-1]:
        at.append(at[-1] + (int(b) + 255) // 256 * 256)
    need = at[-1] + int(sizes[-1]) + 256
    if out is None or out.nbytes < need:
        out = DevBuffer(need, device=device)
    return out, [out.at(o) for o in at], at


def _dev_fetch(out, at, arrays):
    """The result arrays copied out of the DevBuffer `out`, where _dev_results put them."""
    for a, o in zip(arrays, at):
        if a.nbytes:
            _check(lib().mts_dev_copy(out.device, None, _ptr(a), out.at(o), a.nbytes, 1), 'mts_dev_copy')
    return arrays


# -- the tails of the two result kinds that detect, correlate, match_templates, residual and match_residual return.  `what` names the
# entry, chunks is (head, n, status) of _host_chunks / _dev_chunks, mid the op's own arguments; the caller keeps what mid points at.
_EVENT_DTYPES = (np.int64, np.int32, np.float32)        # row; position or template; amplitude or score


def _host_events(what, chunks, mid, cap, n_ev):
    """-> (status list, n_events, the first min(n_events, cap) events as three arrays)."""
    head, n, status = chunks
    res = [np.empty(cap, t) for t in _EVENT_DTYPES]
    _check(getattr(lib(), what)(*head, *mid, *(_ptr(a) if cap else None for a in res), _lp(n_ev), _ip(status)), what)
    k = min(int(n_ev[0]), cap)
    return (_status(status, n), int(n_ev[0])) + tuple(a[:k] for a in res)


def _dev_events(what, cbuf, chunks, mid, cap, n_ev, out, download):
    """-> (status list, n_events, the three arrays or None, out)."""
    head, n, status = chunks
    out, ptrs, at = _dev_results(out, cbuf.device, [cap * np.dtype(t).itemsize for t in _EVENT_DTYPES])
    _check(getattr(lib(), what)(*head, *mid, *ptrs, _lp(n_ev), _ip(status)), what)
    res = None
    if download:
        res = tuple(_dev_fetch(out, at, [np.empty(min(int(n_ev[0]), cap), t) for t in _EVENT_DTYPES]))
    return _status(status, n), int(n_ev[0]), res, out


def _host_dense(what, chunks, mid, shape):
    """-> (status list, the float32 result of `shape`)."""
    head, n, status = chunks
    out = np.empty(shape, np.float32)
    _check(getattr(lib(), what)(*head, *mid, _ptr(out), _ip(status)), what)
    return _status(status, n), out


def _dev_dense(what, cbuf, chunks, mid, shape, out, download):
    """-> (status list, the float32 result of `shape` or None, out)."""
    head, n, status = chunks
    out, ptrs, at = _dev_results(out, cbuf.device, [4 * shape[0] * shape[1]])
    _check(getattr(lib(), what)(*head, *mid, *ptrs, _ip(status)), what)
    res = _dev_fetch(out, at, [np.empty(shape, np.float32)])[0] if download else None
    return _status(status, n), res, out


# -- per-window statistics
def stats_exact(dtype):
    """1- and 2-byte integers: the sum of squares is the exact uint64 sum (converted to float64 once, by the caller)."""
    dtype = np.dtype(dtype)
    return dtype.kind in 'iu' and dtype.itemsize <= 2


def stats_dtypes(dtype):
    """(min/max, sum, sumsq) dtypes of the partial results of one call."""
    dtype = np.dtype(dtype)
    return dtype, np.dtype(np.float64 if dtype.kind == 'f' else np.int64), np.dtype(np.uint64 if stats_exact(dtype) else np.float64)


def _n_windows(row_begin, row_end, window_rows):
    return max(0, -(-(int(row_end) - int(row_begin)) // int(window_rows))) if int(window_rows) >= 1 else 0


def _stats_args(dtype, row_begin, row_end, window_rows, cols):
    """-> (the op's own arguments of mts_window_stats, the arrays min, max, sum, sumsq, the count array, n_windows)."""
    cols = _cols32(cols)
    nw = _n_windows(row_begin, row_end, window_rows)
    t, s, q = stats_dtypes(dtype)
    shape = (nw, int(cols.size))
    res = (np.empty(shape, t), np.empty(shape, t), np.empty(shape, s), np.empty(shape, q))
    return (int(row_begin), int(row_end), int(window_rows), int(cols.size), _ip(cols)), res, np.zeros(max(nw, 1), np.int64), nw


def window_stats(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, row_begin, row_end, window_rows, cols, device=0):
    """mts_window_stats: per-window statistics of the chunks `keys` (file rows [row0[i], row0[i] + n_rows[i])).  cache_id 0: no cache,
    every chunk comes with its bytes; else chunks with lens[i] == 0 must be resident (HipError E_MISS).  Returns (status list,
    Bunch-like dict min, max, sum, sumsq, count) -- the partials of these chunks: sumsq is uint64 for 1/2-byte integers."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, res, cnt, nw = _stats_args(dtype, row_begin, row_end, window_rows, cols)
    _check(lib().mts_window_stats(*head, *mid, *map(_ptr, res), _lp(cnt), _ip(status)), 'mts_window_stats')
    return _status(status, n), dict(zip(('min', 'max', 'sum', 'sumsq'), res), count=cnt[:nw])


def dev_window_stats(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, row_begin, row_end, window_rows, cols, out=None):
    """mts_dev_window_stats on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the four result arrays
    (made when None; returned so that a caller timing repeated calls can pass it again).  Returns (status list, dict of numpy
    arrays as window_stats, out)."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, res, cnt, nw = _stats_args(dtype, row_begin, row_end, window_rows, cols)
    out, ptrs, at = _dev_results(out, cbuf.device, [a.nbytes for a in res])
    _check(lib().mts_dev_window_stats(*head, *mid, *ptrs, _lp(cnt), _ip(status)), 'mts_dev_window_stats')
    _dev_fetch(out, at, res)
    return _status(status, n), dict(zip(('min', 'max', 'sum', 'sumsq'), res), count=cnt[:nw]), out


# -- order statistics: one round of a radix select
RANK_BITS = 8                # digit width (MTS_RANK_BITS)
RANK_SELECTORS = 2           # selectors per (window, column) cell and call (MTS_RANK_SELECTORS)
RANK_KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)      # kmin of a selector without candidates (its kmax is 0)


def rank_key_bits(dtype, mode=0):
    """Significant bits of the order keys: the item's own width in mode 0, 64 in modes 1 and 2 (float64 keys)."""
    return 64 if mode else 8 * np.dtype(dtype).itemsize


def rank_key_nan(dtype, mode=0):
    """The key every NaN maps to (all ones): kmax of a prefix-free selector equals it exactly when the cell holds a NaN."""
    return np.uint64((1 << rank_key_bits(dtype, mode)) - 1)


def _float_keys(x):
    x = np.ascontiguousarray(x)
    u = np.dtype('u%d' % x.dtype.itemsize).type
    b = x.view(u)
    sign = u(1 << (8 * x.dtype.itemsize - 1))
    k = np.where(b & sign, ~b, b | sign)
    k = np.where(x == 0, sign, k)                                 # -0 and +0: one key
    k = np.where(np.isnan(x), u(sign | (sign - u(1))), k)         # every NaN, of either sign: all ones
    return k.astype(np.uint64)


def rank_keys(x, mode=0, center=None):
    """The order keys of mts_rank_hist as uint64 (their unsigned order is np.sort's order of the items).  mode 0: the items in their
    own type -- unsigned: the value; signed: the sign bit flipped; floats: NaN -> all ones, -0 and +0 -> one key, negative numbers'
    bits inverted, the others' sign bit set.  mode 1: the float64 x.astype(float64) - center, mode 2: its absolute value (center
    broadcasts against x; None is 0)."""
    x = np.asarray(x)
    if mode:
        with np.errstate(invalid='ignore', over='ignore'):
            d = x.astype(np.float64) - (0.0 if center is None else np.asarray(center, dtype=np.float64))
        return _float_keys(np.abs(d) if mode == 2 else d)
    if x.dtype.kind == 'f':
        return _float_keys(x)
    if x.dtype.kind == 'u':
        return x.astype(np.uint64)
    u = np.dtype('u%d' % x.dtype.itemsize)
    return np.ascontiguousarray(x).view(u).astype(np.uint64) ^ np.uint64(1 << (8 * x.dtype.itemsize - 1))


def rank_values(keys, dtype, mode=0):
    """The inverse of rank_keys: the items (mode 0, in `dtype`) or the float64 differences (modes 1, 2) that the keys stand for; the
    all-ones key gives NaN, the key of the zeros +0."""
    dtype = np.dtype(np.float64 if mode else dtype)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    u = np.dtype('u%d' % dtype.itemsize)
    k = keys.astype(u)
    sign = u.type(1 << (8 * dtype.itemsize - 1))
    if dtype.kind == 'u':
        return k
    if dtype.kind == 'i':
        return (k ^ sign).view(dtype)
    out = np.where(k & sign, k & ~sign, ~k).view(dtype).copy()
    out[keys == rank_key_nan(dtype)] = np.nan
    return out


def rank_bit_length(x):
    """int.bit_length of every entry of a uint64 array, as uint64: the keys of a round's candidates agree above bit
    rank_bit_length(kmin ^ kmax)."""
    x = np.asarray(x, dtype=np.uint64)
    d = np.zeros(x.shape, np.uint64)
    for b in (32, 16, 8, 4, 2, 1):
        m = (x >> np.uint64(b)) != 0
        d += np.where(m, np.uint64(b), np.uint64(0))
        x = np.where(m, x >> np.uint64(b), x)
    return d + (x != 0).astype(np.uint64)


def _rank_args(row_begin, row_end, window_rows, cols, mode, center, sel_prefix, sel_shift):
    """-> (the op's own arguments of mts_rank_hist, the arrays hist, kmin, kmax, the count array, n_windows)."""
    cols = _cols32(cols)
    nw = _n_windows(row_begin, row_end, window_rows)
    shape = (nw, RANK_SELECTORS, int(cols.size))
    pre = np.ascontiguousarray(sel_prefix, dtype=np.uint64)
    shf = np.ascontiguousarray(sel_shift, dtype=np.int32)
    assert pre.shape == shape and shf.shape == shape, 'selectors must be (n_windows, %d, n_cols)' % RANK_SELECTORS
    cen = None
    if mode:
        cen = _dp(np.ascontiguousarray(np.broadcast_to(np.asarray(0.0 if center is None else center, dtype=np.float64), (shape[0], shape[2]))))
    res = (np.zeros((shape[0], RANK_SELECTORS, 1 << RANK_BITS, shape[2]), np.uint32), np.full(shape, RANK_KEY_NONE, np.uint64),
           np.zeros(shape, np.uint64))
    mid = (int(row_begin), int(row_end), int(window_rows), int(cols.size), _ip(cols), int(mode), cen, _ullp(pre), _ip(shf))
    return mid, res, np.zeros(max(nw, 1), np.int64), nw


def rank_hist(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, row_begin, row_end, window_rows, cols, mode, center,
              sel_prefix, sel_shift, device=0):
    """mts_rank_hist: one round of the radix select over the chunks `keys` (file rows [row0[i], row0[i] + n_rows[i])) on the grid of
    window_stats.  sel_prefix / sel_shift: (n_windows, RANK_SELECTORS, n_cols); shift < 0 marks an inactive selector; the candidates of
    the others are the cell's items with rank_keys(x, mode, center) >> (shift + 8) == prefix.  cache_id 0: no cache, every chunk comes
    with its bytes; else chunks with lens[i] == 0 must be resident (HipError E_MISS).  Returns (status list, dict hist (n_windows, 2,
    256, n_cols) uint32, kmin, kmax (n_windows, 2, n_cols) uint64, count) -- the partials of these chunks: integers, to be added
    (hist, count) and combined with minimum / maximum (kmin, kmax) in any order."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, (hist, kmin, kmax), cnt, nw = _rank_args(row_begin, row_end, window_rows, cols, mode, center, sel_prefix, sel_shift)
    _check(lib().mts_rank_hist(*head, *mid, hist.ctypes.data_as(C.POINTER(C.c_uint)), _ullp(kmin), _ullp(kmax), _lp(cnt), _ip(status)),
           'mts_rank_hist')
    return _status(status, n), dict(hist=hist, kmin=kmin, kmax=kmax, count=cnt[:nw])


def dev_rank_hist(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, row_begin, row_end, window_rows, cols, mode, center, sel_prefix,
                  sel_shift, out=None, fetch=True):
    """mts_dev_rank_hist on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the three result arrays (made
    when None; returned so that a caller timing repeated calls can pass it again); fetch=False leaves them there.  Returns (status
    list, dict as rank_hist, out)."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, res, cnt, nw = _rank_args(row_begin, row_end, window_rows, cols, mode, center, sel_prefix, sel_shift)
    out, ptrs, at = _dev_results(out, cbuf.device, [a.nbytes for a in res])
    _check(lib().mts_dev_rank_hist(*head, *mid, *ptrs, _lp(cnt), _ip(status)), 'mts_dev_rank_hist')
    if fetch:
        _dev_fetch(out, at, res)
    return _status(status, n), dict(zip(('hist', 'kmin', 'kmax'), res), count=cnt[:nw]), out


# -- the same round over the filtered signal z of detect
ZRANK_BLOCK_ROWS = 4096      # rows of z that one workgroup of k_zrank_hist counts (ZSEL_BLOCK_ROWS)


def _frank_args(valid_begin, valid_end, taps, cols, reference, row_begin, row_end, window_rows, count_begin, count_end, mode, center, sel_prefix,
                sel_shift):
    """-> (the op's own arguments of mts_filtered_rank_hist, the arrays hist, kmin, kmax, the count array, n_windows)."""
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).ravel())
    grid, res, cnt, nw = _rank_args(row_begin, row_end, window_rows, cols, mode, center, sel_prefix, sel_shift)
    mid = (int(valid_begin), int(valid_end), int(taps.size), _dp(taps)) + grid[3:5] + (int(reference),) + grid[:3] + (
        int(count_begin), int(count_end)) + grid[5:]
    return mid, res, cnt, nw


def filtered_rank_hist(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference,
                       row_begin, row_end, window_rows, count_begin, count_end, mode, center, sel_prefix, sel_shift, device=0):
    """mts_filtered_rank_hist: one round of the radix select over z, the filtered rows of mts_detect (taps, cols, reference 0 / 1,
    float32 items), from the adjacent chunks `keys`.  The grid (row_begin, row_end, window_rows), mode, center and the selectors as
    rank_hist for a float32 recording; only the rows of [count_begin, count_end), inside the grid, are counted, and the chunks cover
    their filter support.  cache_id 0: no cache, every chunk comes with its bytes; else chunks with lens[i] == 0 must be resident
    (HipError E_MISS).  Returns (status list, dict hist, kmin, kmax, count as rank_hist): partials to be added and combined in any
    order, to be discarded when a status is not CHUNK_OK."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, (hist, kmin, kmax), cnt, nw = _frank_args(valid_begin, valid_end, taps, cols, reference, row_begin, row_end, window_rows, count_begin,
                                                   count_end, mode, center, sel_prefix, sel_shift)
    _check(lib().mts_filtered_rank_hist(*head, *mid, hist.ctypes.data_as(C.POINTER(C.c_uint)), _ullp(kmin), _ullp(kmax), _lp(cnt), _ip(status)),
           'mts_filtered_rank_hist')
    return _status(status, n), dict(hist=hist, kmin=kmin, kmax=kmax, count=cnt[:nw])


def dev_filtered_rank_hist(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference, row_begin,
                           row_end, window_rows, count_begin, count_end, mode, center, sel_prefix, sel_shift, out=None, fetch=True):
    """mts_dev_filtered_rank_hist on a DevBuffer of compressed chunks (offsets into it).  `out`, fetch and the result as dev_rank_hist."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, res, cnt, nw = _frank_args(valid_begin, valid_end, taps, cols, reference, row_begin, row_end, window_rows, count_begin, count_end, mode,
                                    center, sel_prefix, sel_shift)
    out, ptrs, at = _dev_results(out, cbuf.device, [a.nbytes for a in res])
    _check(lib().mts_dev_filtered_rank_hist(*head, *mid, *ptrs, _lp(cnt), _ip(status)), 'mts_dev_filtered_rank_hist')
    if fetch:
        _dev_fetch(out, at, res)
    return _status(status, n), dict(zip(('hist', 'kmin', 'kmax'), res), count=cnt[:nw]), out


# -- FIR low-pass + decimation
DECIMATE_MAX_TAPS = 8192


def _dec_args(valid_begin, valid_end, first_row, n_out, q, taps, out_dtype, cols):
    """-> (the op's own arguments of mts_decimate, the shape of the result, its dtype)."""
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).ravel())
    out_dtype = np.dtype(out_dtype)
    cols = _cols32(cols)
    mid = (int(valid_begin), int(valid_end), int(first_row), int(n_out), int(q), int(taps.size), _dp(taps), out_dtype.itemsize,
           int(cols.size), _ip(cols))
    return mid, (max(int(n_out), 0), int(cols.size)), out_dtype


def decimate(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, first_row, n_out, q, taps,
             out_dtype, cols, device=0):
    """mts_decimate: y[k, c] = sum_j taps[j] * x[first_row + k * q - j, cols[c]] (x = 0 outside [valid_begin, valid_end)) for k < n_out,
    from the adjacent chunks `keys` (file rows [row0[i], row0[i] + n_rows[i])).  cache_id 0: no cache, every chunk comes with its
    bytes; else chunks with lens[i] == 0 must be resident (HipError E_MISS).  Returns (status list, (n_out, n_cols) out_dtype)."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, shape, out_dtype = _dec_args(valid_begin, valid_end, first_row, n_out, q, taps, out_dtype, cols)
    out = np.empty(shape, out_dtype)
    _check(lib().mts_decimate(*head, *mid, _ptr(out), _ip(status)), 'mts_decimate')
    return _status(status, n), out


def dev_decimate(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, first_row, n_out, q, taps, out_dtype, cols,
                 out=None, download=True):
    """mts_dev_decimate on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the result (made when None;
    returned so that a caller timing repeated calls can pass it again).  Returns (status list, numpy array or None, out)."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, shape, out_dtype = _dec_args(valid_begin, valid_end, first_row, n_out, q, taps, out_dtype, cols)
    out, ptrs, at = _dev_results(out, cbuf.device, [shape[0] * shape[1] * out_dtype.itemsize])
    _check(lib().mts_dev_decimate(*head, *mid, *ptrs, _ip(status)), 'mts_dev_decimate')
    res = _dev_fetch(out, at, [np.empty(shape, out_dtype)])[0] if download else None
    return _status(status, n), res, out


# -- channel-mixing matrix products
PROJECT_MAX_COLS = 1024                # MTS_PROJECT_MAX_COLS
PROJECT_MAX_OUT = 1024                 # MTS_PROJECT_MAX_OUT


def _proj_args(row_begin, row_end, cols, offset, weights, out_dtype):
    """-> (the op's own arguments of mts_project, the shape of the result, its dtype)."""
    cols = _cols32(cols)
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
    assert w.ndim == 2 and w.shape[0] == cols.size, 'weights must be (n_cols, n_out)'
    off = None if offset is None else np.ascontiguousarray(np.broadcast_to(np.asarray(offset, dtype=np.float64), (cols.size,)))
    out_dtype = np.dtype(out_dtype)
    mid = (int(row_begin), int(row_end), int(cols.size), _ip(cols), None if off is None else _dp(off), int(w.shape[1]), _dp(w),
           out_dtype.itemsize)
    return mid, (max(int(row_end) - int(row_begin), 0), int(w.shape[1])), out_dtype, (cols, off, w)


def project(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, row_begin, row_end, cols, offset, weights, out_dtype,
            device=0):
    """mts_project: y[t, k] = sum_j (x[t, cols[j]] - offset[j]) * weights[j, k] for file rows [row_begin, row_end), from the adjacent
    chunks `keys` (file rows [row0[i], row0[i] + n_rows[i])); weights (n_cols, n_out), offset None, a scalar or (n_cols,).  cache_id 0:
    no cache, every chunk comes with its bytes; else chunks with lens[i] == 0 must be resident (HipError E_MISS).  Returns (status
    list, (row_end - row_begin, n_out) out_dtype)."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, shape, out_dtype, _keep = _proj_args(row_begin, row_end, cols, offset, weights, out_dtype)
    out = np.empty(shape, out_dtype)
    _check(lib().mts_project(*head, *mid, _ptr(out), _ip(status)), 'mts_project')
    return _status(status, n), out


def dev_project(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, row_begin, row_end, cols, offset, weights, out_dtype, out=None,
                download=True):
    """mts_dev_project on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the result (made when None;
    returned so that a caller timing repeated calls can pass it again).  Returns (status list, numpy array or None, out)."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, shape, out_dtype, _keep = _proj_args(row_begin, row_end, cols, offset, weights, out_dtype)
    out, ptrs, at = _dev_results(out, cbuf.device, [shape[0] * shape[1] * out_dtype.itemsize])
    _check(lib().mts_dev_project(*head, *mid, *ptrs, _ip(status)), 'mts_dev_project')
    res = _dev_fetch(out, at, [np.empty(shape, out_dtype)])[0] if download else None
    return _status(status, n), res, out


# -- threshold-crossing peak detection
DETECT_MAX_EXCLUDE = 255
DETECT_MAX_SPREAD = 32
DETECT_MAX_REF_COLS = 1024
DETECT_SIGNS = {'neg': 0, 'pos': 1, 'both': 2}


def _det_args(valid_begin, valid_end, row_begin, row_end, taps, cols, threshold, sign, reference, exclude_rows, exclude_cols, max_events):
    """-> (the op's own arguments of mts_detect, the events the buffers hold, the array for n_events)."""
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).ravel())
    cols = _cols32(cols)
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(threshold, dtype=np.float32), (cols.size,)))
    mid = (int(valid_begin), int(valid_end), int(row_begin), int(row_end), int(taps.size), _dp(taps), int(cols.size), _ip(cols),
           thr.ctypes.data_as(C.POINTER(C.c_float)), int(sign), int(reference), int(exclude_rows), int(exclude_cols), int(max_events))
    return mid, max(int(max_events), 0), np.zeros(1, np.int64)


def detect(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end, taps, cols,
           threshold, sign, reference, exclude_rows, exclude_cols, max_events, device=0):
    """mts_detect: the events of rows [row_begin, row_end) (include/mtscomp_hip.h) from the adjacent chunks `keys`.  sign 0 / 1 / 2,
    reference 0 / 1.  cache_id 0: no cache, every chunk comes with its bytes; else chunks with lens[i] == 0 must be resident (HipError
    E_MISS).  Returns (status list, n_events, row int64, pos int32, amp float32): the first min(n_events, max_events) events."""
    mid, cap, n_ev = _det_args(valid_begin, valid_end, row_begin, row_end, taps, cols, threshold, sign, reference, exclude_rows, exclude_cols,
                               max_events)
    return _host_events('mts_detect', _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags), mid, cap, n_ev)


def dev_detect(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end, taps, cols, threshold, sign,
               reference, exclude_rows, exclude_cols, max_events, out=None, download=True):
    """mts_dev_detect on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the three event arrays (made when
    None; returned so that a caller timing repeated calls can pass it again).  Returns (status list, n_events, (row, pos, amp) or None,
    out)."""
    mid, cap, n_ev = _det_args(valid_begin, valid_end, row_begin, row_end, taps, cols, threshold, sign, reference, exclude_rows, exclude_cols,
                               max_events)
    return _dev_events('mts_dev_detect', cbuf, _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags), mid, cap, n_ev, out, download)


# -- snippets around events and their extrema
WAVEFORMS_MAX_ROWS = 4096
WAVEFORMS_MAX_WIDTH = 1024
_WAVEFORMS_DTYPES = (np.float32, np.int32, np.float32, np.int32)       # min, argmin, max, argmax of an event


def _wav_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width):
    """-> (the op's own arguments of mts_waveforms, the events, the entries of a snippet)."""
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).ravel())
    cols = _cols32(cols)
    ev_row = _longs(ev_row)
    ev_col0 = np.ascontiguousarray(np.asarray(ev_col0, dtype=np.int32))
    assert ev_row.ndim == 1 and ev_row.shape == ev_col0.shape
    mid = (int(valid_begin), int(valid_end), int(taps.size), _dp(taps), int(cols.size), _ip(cols), int(reference), int(ev_row.size), _lp(ev_row),
           _ip(ev_col0), int(before), int(after), int(width))
    return mid, int(ev_row.size), max(int(before) + int(after), 0) * max(int(width), 0)


def waveforms(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference, ev_row,
              ev_col0, before, after, width, want_wave=True, device=0):
    """mts_waveforms: the snippets (before + after rows x width positions) of the events at the ascending file rows ev_row with first
    column positions ev_col0 (include/mtscomp_hip.h) from the adjacent chunks `keys`.  reference 0 / 1.  cache_id 0: no cache, every
    chunk comes with its bytes; else chunks with lens[i] == 0 must be resident (HipError E_MISS).  Returns (status list, wave float32
    (n, T, width) or None without want_wave, min float32, argmin int32, max float32, argmax int32)."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, n_ev, item = _wav_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width)
    wave = np.empty((n_ev, int(before) + int(after), int(width)) if item else (n_ev, 0, 0), np.float32) if want_wave else None
    res = [np.empty(n_ev, t) for t in _WAVEFORMS_DTYPES]
    _check(lib().mts_waveforms(*head, *mid, _ptr(wave) if want_wave else None, *(_ptr(a) for a in res), _ip(status)), 'mts_waveforms')
    return (_status(status, n), wave) + tuple(res)


def dev_waveforms(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before,
                  after, width, want_wave=True, out=None, download=True):
    """mts_dev_waveforms on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the snippets and the four
    extrema arrays (made when None; returned so that a caller timing repeated calls can pass it again).  Returns (status list,
    (wave or None, min, argmin, max, argmax) or None, out)."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, n_ev, item = _wav_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width)
    sizes = [4 * n_ev * item if want_wave else 0] + [4 * n_ev] * 4
    out, ptrs, at = _dev_results(out, cbuf.device, sizes)
    _check(lib().mts_dev_waveforms(*head, *mid, ptrs[0] if want_wave else None, *ptrs[1:], _ip(status)), 'mts_dev_waveforms')
    res = None
    if download:
        wave = np.empty((n_ev, int(before) + int(after), int(width)), np.float32) if want_wave else np.empty(0, np.float32)
        got = _dev_fetch(out, at, [wave] + [np.empty(n_ev, t) for t in _WAVEFORMS_DTYPES])
        res = (got[0] if want_wave else None,) + tuple(got[1:])
    return _status(status, n), res, out


def waveforms_last_plan(device=0):
    """What the last waveforms call on `device` did: a dict of pieces, slabs, gap_cuts (slabs begun at a gap) and gather_us (the gather
    kernels' microseconds, measured only while MTS_WAVEFORMS_TIME is set)."""
    out = np.zeros(4, np.int64)
    _check(lib().mts_waveforms_last_plan(int(device), _lp(out)), 'mts_waveforms_last_plan')
    return dict(zip(('pieces', 'slabs', 'gap_cuts', 'gather_us'), (int(v) for v in out)))


# -- per-label fixed-point sums of those snippets
MEAN_MAX_LABELS = 4096                 # MTS_MEAN_MAX_LABELS
MEAN_MAX_ENTRIES = 1 << 27             # MTS_MEAN_MAX_ENTRIES
MEAN_MAX_LABEL_EVENTS = 1 << 21        # events of one label in a call
_MEAN_DTYPES = (np.int64, np.int32, np.int64)                           # sum, count, skipped


def mean_resolution_ok(resolution):
    """A power of two in [2^-60, 2^60]: what mts_mean_waveforms takes for its fixed point."""
    try:
        m, e = math.frexp(float(resolution))
    except (TypeError, ValueError, OverflowError):
        return False
    return m == 0.5 and -60 <= e - 1 <= 60


def _mean_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, ev_label, n_labels, before, after, width, resolution):
    """-> (the op's own arguments of mts_mean_waveforms, the shapes of its three results)."""
    wav, _, item = _wav_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width)
    ev_label = np.ascontiguousarray(np.asarray(ev_label, dtype=np.int32))
    assert ev_label.ndim == 1 and ev_label.size == wav[7]
    mid = wav[:10] + (_ip(ev_label), int(n_labels)) + wav[10:] + (float(resolution),)
    K = max(int(n_labels), 0)
    shape = (K, int(before) + int(after), int(width)) if item else (K, 0, 0)
    return mid, (shape, shape, (K,))


def mean_waveforms(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference,
                   ev_row, ev_col0, ev_label, n_labels, before, after, width, resolution, device=0):
    """mts_mean_waveforms: the fixed-point sums over each label's events of the snippets that mts_waveforms would return for them
    (include/mtscomp_hip.h), from the adjacent chunks `keys`.  ev_label: ints in [0, n_labels).  cache_id as waveforms.  Returns
    (status list, sum int64 (n_labels, T, width), count int32 (n_labels, T, width), skipped int64 (n_labels))."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, shapes = _mean_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, ev_label, n_labels, before, after, width, resolution)
    res = [np.empty(sh, t) for sh, t in zip(shapes, _MEAN_DTYPES)]
    _check(lib().mts_mean_waveforms(*head, *mid, *(_ptr(a) for a in res), _ip(status)), 'mts_mean_waveforms')
    return (_status(status, n),) + tuple(res)


def dev_mean_waveforms(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0,
                       ev_label, n_labels, before, after, width, resolution, out=None, download=True):
    """mts_dev_mean_waveforms on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the three results (made
    when None; returned so that a caller timing repeated calls can pass it again).  Returns (status list, (sum, count, skipped) or
    None, out)."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, shapes = _mean_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, ev_label, n_labels, before, after, width, resolution)
    res = [np.empty(sh, t) for sh, t in zip(shapes, _MEAN_DTYPES)]
    out, ptrs, at = _dev_results(out, cbuf.device, [a.nbytes for a in res])
    _check(lib().mts_dev_mean_waveforms(*head, *mid, *ptrs, _ip(status)), 'mts_dev_mean_waveforms')
    return _status(status, n), tuple(_dev_fetch(out, at, res)) if download else None, out


# -- those snippets projected on a temporal basis
FEATURES_MAX_COMPONENTS = 32           # MTS_FEATURES_MAX_COMPONENTS
FEATURES_MAX_BASIS = 8192              # MTS_FEATURES_MAX_BASIS


def _feat_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width, basis):
    """-> (the op's own arguments of mts_waveform_features, the shape of its result, the basis that the pointer among them points into)."""
    wav, n_ev, item = _wav_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width)
    basis = np.ascontiguousarray(np.asarray(basis, dtype=np.float32))
    assert basis.ndim == 2 and basis.shape[1] == int(before) + int(after)
    mid = wav + (int(basis.shape[0]), basis.ctypes.data_as(C.POINTER(C.c_float)))
    return mid, ((n_ev, int(basis.shape[0]), int(width)) if item else (n_ev, 0, 0)), basis


def waveform_features(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference,
                      ev_row, ev_col0, before, after, width, basis, device=0):
    """mts_waveform_features: the snippets that mts_waveforms would return for the events, each column (e, ., w) projected on the rows of
    basis (n_comp, before + after) float32 by a chain of fmaf (include/mtscomp_hip.h), from the adjacent chunks `keys`.  cache_id as
    waveforms.  Returns (status list, features float32 (n, n_comp, width))."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, shape, basis = _feat_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width, basis)
    feat = np.empty(shape, np.float32)
    _check(lib().mts_waveform_features(*head, *mid, _ptr(feat), _ip(status)), 'mts_waveform_features')
    return _status(status, n), feat


def dev_waveform_features(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0,
                          before, after, width, basis, out=None, download=True):
    """mts_dev_waveform_features on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the features (made when
    None; returned so that a caller timing repeated calls can pass it again).  Returns (status list, features or None, out)."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, shape, basis = _feat_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width, basis)
    feat = np.empty(shape, np.float32)
    out, ptrs, at = _dev_results(out, cbuf.device, [feat.nbytes])
    _check(lib().mts_dev_waveform_features(*head, *mid, *ptrs, _ip(status)), 'mts_dev_waveform_features')
    return _status(status, n), _dev_fetch(out, at, [feat])[0] if download else None, out


# -- those snippets reduced to channel amplitudes and amplitude-weighted position sums
LOCALIZE_MAX_DIMS = 4                  # MTS_LOCALIZE_MAX_DIMS
LOCALIZE_MODES = {'ptp': 0, 'neg': 1, 'pos': 2, 'abs': 3}               # MTS_LOCALIZE_PTP, _NEG, _POS, _ABS
_LOCALIZE_DTYPES = (np.float32, np.float32, np.int32)                   # weight, moment, best of an event


def _loc_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width, mode, positions):
    """-> (the op's own arguments of mts_localize, the shapes of its four results, the positions that the pointer among them points
    into)."""
    wav, n_ev, _ = _wav_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width)
    positions = np.ascontiguousarray(np.asarray(positions, dtype=np.float32))
    assert positions.ndim == 2 and positions.shape[0] == wav[4]
    D = int(positions.shape[1])
    mid = wav + (int(mode), D, positions.ctypes.data_as(C.POINTER(C.c_float)))
    return mid, ((n_ev, max(int(width), 0)), (n_ev,), (n_ev, D), (n_ev,)), positions


def localize(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference, ev_row,
             ev_col0, before, after, width, mode, positions, want_amp=True, device=0):
    """mts_localize: the snippets that mts_waveforms would return for the events reduced to the amplitude of every column (mode 0 .. 3:
    LOCALIZE_MODES) and the chains weight = sum g, moment = sum g * positions[c] over the amplitudes g > 0 (include/mtscomp_hip.h), from
    the adjacent chunks `keys`.  positions: (n_cols, n_dims) float32.  cache_id as waveforms.  Returns (status list, amplitude float32
    (n, width) or None without want_amp, weight float32 (n), moment float32 (n, n_dims), best int32 (n))."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, shapes, positions = _loc_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width, mode, positions)
    amp = np.empty(shapes[0], np.float32) if want_amp else None
    res = [np.empty(sh, t) for sh, t in zip(shapes[1:], _LOCALIZE_DTYPES)]
    _check(lib().mts_localize(*head, *mid, _ptr(amp) if want_amp else None, *(_ptr(a) for a in res), _ip(status)), 'mts_localize')
    return (_status(status, n), amp) + tuple(res)


def dev_localize(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0,
                 before, after, width, mode, positions, want_amp=True, out=None, download=True):
    """mts_dev_localize on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the four results (made when
    None; returned so that a caller timing repeated calls can pass it again).  Returns (status list, (amplitude or None, weight,
    moment, best) or None, out)."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, shapes, positions = _loc_args(valid_begin, valid_end, taps, cols, reference, ev_row, ev_col0, before, after, width, mode, positions)
    amp = np.empty(shapes[0] if want_amp else 0, np.float32)
    res = [amp] + [np.empty(sh, t) for sh, t in zip(shapes[1:], _LOCALIZE_DTYPES)]
    out, ptrs, at = _dev_results(out, cbuf.device, [a.nbytes for a in res])
    _check(lib().mts_dev_localize(*head, *mid, ptrs[0] if want_amp else None, *ptrs[1:], _ip(status)), 'mts_dev_localize')
    got = None
    if download:
        got = _dev_fetch(out, at, res)
        got = (got[0] if want_amp else None,) + tuple(got[1:])
    return _status(status, n), got, out


# -- spatio-temporal template scores
CORRELATE_MAX_T = 256                  # MTS_CORRELATE_MAX_T
CORRELATE_MAX_OUT = 1024               # MTS_CORRELATE_MAX_OUT
CORRELATE_MAX_COLS = 1024              # MTS_CORRELATE_MAX_COLS


def _cor_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates):
    """-> (the op's own arguments of mts_correlate, the shape of the result, what the pointers point at)."""
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).ravel())
    cols = _cols32(cols)
    with np.errstate(over='ignore'):
        tpl = np.ascontiguousarray(np.asarray(templates).astype(np.float32))
    assert tpl.ndim == 3 and tpl.shape[2] == cols.size, 'templates must be (n_out, T, n_cols)'
    mid = (int(valid_begin), int(valid_end), int(row_begin), int(row_end), int(taps.size), _dp(taps), int(cols.size), _ip(cols), int(reference),
           int(before), int(tpl.shape[1]), int(tpl.shape[0]), tpl.ctypes.data_as(C.POINTER(C.c_float)))
    return mid, (max(int(row_end) - int(row_begin), 0), int(tpl.shape[0])), (taps, cols, tpl)


def correlate(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end, taps, cols,
              reference, before, templates, device=0):
    """mts_correlate: score[t, k] of the templates (n_out, T, n_cols), template row `before` on file row t, for file rows [row_begin,
    row_end) (include/mtscomp_hip.h) from the adjacent chunks `keys`.  reference 0 / 1.  cache_id 0: no cache, every chunk comes with
    its bytes; else chunks with lens[i] == 0 must be resident (HipError E_MISS).  Returns (status list, (row_end - row_begin, n_out)
    float32)."""
    mid, shape, _keep = _cor_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates)
    return _host_dense('mts_correlate', _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags), mid, shape)


def dev_correlate(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end, taps, cols, reference,
                  before, templates, out=None, download=True):
    """mts_dev_correlate on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the scores (made when None;
    returned so that a caller timing repeated calls can pass it again).  Returns (status list, numpy array or None, out)."""
    mid, shape, _keep = _cor_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates)
    return _dev_dense('mts_dev_correlate', cbuf, _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags), mid, shape, out, download)


# -- template-matching events
TMATCH_MAX_EXCLUDE = 255               # MTS_TMATCH_MAX_EXCLUDE


def _tm_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates, threshold, exclude_rows, max_events):
    """-> (the op's own arguments of mts_match_templates, the events the buffers hold, the array for n_events, what the pointers point at)."""
    mid, shape, keep = _cor_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates)
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(threshold, dtype=np.float32), (shape[1],)))
    mid = mid + (thr.ctypes.data_as(C.POINTER(C.c_float)), int(exclude_rows), int(max_events))
    return mid, max(int(max_events), 0), np.zeros(1, np.int64), keep + (thr,)


def match_templates(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end, taps,
                    cols, reference, before, templates, threshold, exclude_rows, max_events, device=0):
    """mts_match_templates: the template events of rows [row_begin, row_end) (include/mtscomp_hip.h) from the adjacent chunks `keys` (none
    when the rows read nothing of the recording).  templates (n_out, T, n_cols), threshold a number or one per template, reference 0 / 1.
    cache_id 0: no cache, every chunk comes with its bytes; else chunks with lens[i] == 0 must be resident (HipError E_MISS).  Returns
    (status list, n_events, row int64, template int32, score float32): the first min(n_events, max_events) events."""
    mid, cap, n_ev, _keep = _tm_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates, threshold, exclude_rows,
                                     max_events)
    return _host_events('mts_match_templates', _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags), mid,
                        cap, n_ev)


def dev_match_templates(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end, taps, cols, reference,
                        before, templates, threshold, exclude_rows, max_events, out=None, download=True):
    """mts_dev_match_templates on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the three event arrays (made
    when None; returned so that a caller timing repeated calls can pass it again).  Returns (status list, n_events, (row, template,
    score) or None, out)."""
    mid, cap, n_ev, _keep = _tm_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates, threshold, exclude_rows,
                                     max_events)
    return _dev_events('mts_dev_match_templates', cbuf, _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags), mid, cap, n_ev, out,
                       download)


# -- template peeling: the filtered rows minus matched templates, and the template events of those rows
RESIDUAL_MAX_EVENTS = 1 << 30          # n_sub of mts_residual and mts_match_residual


def _sub_args(sub_row, sub_tpl, sub_amp):
    """-> (n_sub and the three pointers of mts_residual / mts_match_residual, what they point at).  The events in row order."""
    row = _longs(sub_row)
    tpl = np.ascontiguousarray(np.asarray(sub_tpl, dtype=np.int32))
    amp = np.ascontiguousarray(np.asarray(sub_amp, dtype=np.float32))
    assert row.ndim == 1 and row.shape == tpl.shape == amp.shape, 'the events are three 1-D arrays of one length'
    n = int(row.size)
    return (n, _lp(row) if n else None, _ip(tpl) if n else None, amp.ctypes.data_as(C.POINTER(C.c_float)) if n else None), (row, tpl, amp)


def _res_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates, sub_row, sub_tpl, sub_amp):
    """-> (the op's own arguments of mts_residual, the shape of the result, what the pointers point at)."""
    mid, shape, keep = _cor_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates)
    sub, keep_sub = _sub_args(sub_row, sub_tpl, sub_amp)
    return mid + sub, (shape[0], int(keep[1].size)), keep + keep_sub


def residual(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end, taps, cols,
             reference, before, templates, sub_row, sub_tpl, sub_amp, device=0):
    """mts_residual: z' of file rows [row_begin, row_end) (include/mtscomp_hip.h) -- the filtered, referenced rows minus sub_amp[e] times
    template sub_tpl[e] laid with its row `before` on file row sub_row[e], for the events in ascending row order -- from the adjacent
    chunks `keys`.  templates (n_out, T, n_cols), reference 0 / 1.  cache_id 0: no cache, every chunk comes with its bytes; else chunks
    with lens[i] == 0 must be resident (HipError E_MISS).  Returns (status list, (row_end - row_begin, n_cols) float32)."""
    mid, shape, _keep = _res_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates, sub_row, sub_tpl, sub_amp)
    return _host_dense('mts_residual', _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags), mid, shape)


def dev_residual(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end, taps, cols, reference,
                 before, templates, sub_row, sub_tpl, sub_amp, out=None, download=True):
    """mts_dev_residual on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the rows (made when None;
    returned so that a caller timing repeated calls can pass it again).  Returns (status list, numpy array or None, out)."""
    mid, shape, _keep = _res_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates, sub_row, sub_tpl, sub_amp)
    return _dev_dense('mts_dev_residual', cbuf, _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags), mid, shape, out, download)


def match_residual(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end, taps,
                   cols, reference, before, templates, threshold, exclude_rows, max_events, sub_row, sub_tpl, sub_amp, device=0):
    """mts_match_residual: match_templates on z' -- the events (sub_row, sub_tpl, sub_amp), in ascending row order, subtracted from the
    filtered rows before they are scored (include/mtscomp_hip.h).  Arguments and result as match_templates."""
    mid, cap, n_ev, _keep = _tm_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates, threshold, exclude_rows,
                                     max_events)
    sub, _keep_sub = _sub_args(sub_row, sub_tpl, sub_amp)
    return _host_events('mts_match_residual', _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags),
                        mid + sub, cap, n_ev)


def dev_match_residual(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, row_begin, row_end, taps, cols, reference,
                       before, templates, threshold, exclude_rows, max_events, sub_row, sub_tpl, sub_amp, out=None, download=True):
    """mts_dev_match_residual on a DevBuffer of compressed chunks (offsets into it); `out` and the result as dev_match_templates."""
    mid, cap, n_ev, _keep = _tm_args(valid_begin, valid_end, row_begin, row_end, taps, cols, reference, before, templates, threshold, exclude_rows,
                                     max_events)
    sub, _keep_sub = _sub_args(sub_row, sub_tpl, sub_amp)
    return _dev_events('mts_dev_match_residual', cbuf, _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags), mid + sub, cap, n_ev,
                       out, download)


# -- Welch power spectral density
WELCH_MAX_NPERSEG = 16384
WELCH_BLOCK_SEGMENTS = 32              # B: segments summed in order on the device (MTS_WELCH_BLOCK_SEGMENTS)
WELCH_GROUP_ROWS = 1 << 20             # G: the smallest multiple of B segments with G * step >= this (MTS_WELCH_GROUP_ROWS)


def welch_group_segments(step):
    """G for a step: the smallest multiple of WELCH_BLOCK_SEGMENTS with G * step >= WELCH_GROUP_ROWS."""
    b = WELCH_BLOCK_SEGMENTS
    return b * -(-WELCH_GROUP_ROWS // (int(step) * b))


def _welch_args(row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend, compute_dtype, cols):
    """-> (the op's own arguments of mts_welch, the shape of the float64 group sums)."""
    taper = np.ascontiguousarray(np.asarray(taper, dtype=np.float64).ravel())
    cols = _cols32(cols)
    mid = (int(row_seg0), int(seg_begin), int(seg_end), int(nperseg), int(step), _dp(taper), int(bool(detrend)),
           np.dtype(compute_dtype).itemsize, int(cols.size), _ip(cols))
    n_groups = -(-(int(seg_end) - int(seg_begin)) // welch_group_segments(step))
    return mid, (max(n_groups, 0), int(nperseg) // 2 + 1, int(cols.size))


def welch(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, row_seg0, seg_begin, seg_end, nperseg, step, taper,
          detrend, compute_dtype, cols, device=0):
    """mts_welch: the group sums of |X_k|^2 (float64, (n_groups, nperseg // 2 + 1, n_cols)) of segments [seg_begin, seg_end), segment s
    covering file rows [row_seg0 + s * step, + nperseg), from the adjacent chunks `keys` (file rows [row0[i], row0[i] + n_rows[i])).
    cache_id 0: no cache, every chunk comes with its bytes; else chunks with lens[i] == 0 must be resident (HipError E_MISS).
    Returns (status list, partials)."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, shape = _welch_args(row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend, compute_dtype, cols)
    out = np.empty(shape, np.float64)
    _check(lib().mts_welch(*head, *mid, _ptr(out), _ip(status)), 'mts_welch')
    return _status(status, n), out


def dev_welch(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend,
              compute_dtype, cols, out=None, download=True):
    """mts_dev_welch on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for the partials (made when None;
    returned so that a caller timing repeated calls can pass it again).  Returns (status list, numpy array or None, out)."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, shape = _welch_args(row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend, compute_dtype, cols)
    out, ptrs, at = _dev_results(out, cbuf.device, [8 * shape[0] * shape[1] * shape[2]])
    _check(lib().mts_dev_welch(*head, *mid, *ptrs, _ip(status)), 'mts_dev_welch')
    res = _dev_fetch(out, at, [np.empty(shape, np.float64)])[0] if download else None
    return _status(status, n), res, out


# -- channel x channel Gram matrices
GRAM_GROUP_ROWS = 1 << 20              # rows per group of a window, aligned to its start (MTS_GRAM_GROUP_ROWS)
GRAM_SLAB_ROWS = 4096                  # rows per slab of a group, aligned to its start (MTS_GRAM_SLAB_ROWS)
GRAM_MAX_COLS = 16384                  # MTS_GRAM_MAX_COLS


def gram_exact(dtype):
    """1- and 2-byte integers: a group's Gram entries are exact int64 (every partial sum is an integer below 2^52)."""
    dtype = np.dtype(dtype)
    return dtype.kind in 'iu' and dtype.itemsize <= 2


def gram_dtypes(dtype):
    """(gram, sum) dtypes of the partial results of one call: int64 Gram entries for 1- and 2-byte integers, float64 otherwise;
    int64 sums (modulo 2^64) for every integer type, float64 for floats."""
    dtype = np.dtype(dtype)
    return np.dtype(np.int64 if gram_exact(dtype) else np.float64), np.dtype(np.float64 if dtype.kind == 'f' else np.int64)


def gram_groups(range_begin, range_end, window_rows):
    """The number of groups of the grid: windows of window_rows rows over [range_begin, range_end), each cut into groups of
    GRAM_GROUP_ROWS rows aligned to its start."""
    n, w = int(range_end) - int(range_begin), int(window_rows)
    k = -(-w // GRAM_GROUP_ROWS)
    return (n // w) * k + -(-(n % w) // GRAM_GROUP_ROWS)


def gram_group_rows(range_begin, range_end, window_rows, g):
    """File rows [lo, hi) of group g of the grid (group g % K of window g // K, K = ceil(window_rows / GRAM_GROUP_ROWS))."""
    w = int(window_rows)
    k = -(-w // GRAM_GROUP_ROWS)
    w0 = int(range_begin) + (g // k) * w
    lo = w0 + (g % k) * GRAM_GROUP_ROWS
    return lo, min(lo + GRAM_GROUP_ROWS, w0 + w, int(range_end))


def _gram_args(dtype, range_begin, range_end, window_rows, group_begin, group_end, cols):
    """-> (the op's own arguments of mts_gram, the shapes and dtypes of the Gram entries and the sums)."""
    cols = _cols32(cols)
    ng, nc = max(int(group_end) - int(group_begin), 0), int(cols.size)
    g_dt, s_dt = gram_dtypes(dtype)
    mid = (int(range_begin), int(range_end), int(window_rows), int(group_begin), int(group_end), nc, _ip(cols))
    return mid, (((ng, nc, nc), g_dt), ((ng, nc), s_dt))


def gram(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, range_begin, range_end, window_rows, group_begin, group_end,
         cols, device=0):
    """mts_gram: the Gram entries and column sums of groups [group_begin, group_end) of the grid (range, window_rows), from the
    adjacent chunks `keys` (file rows [row0[i], row0[i] + n_rows[i])).  cache_id 0: no cache, every chunk comes with its bytes; else
    chunks with lens[i] == 0 must be resident (HipError E_MISS).  Returns (status list, gram (n_groups, n_cols, n_cols), sum (n_groups,
    n_cols)) in the gram_dtypes of the recording's dtype."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, outs = _gram_args(dtype, range_begin, range_end, window_rows, group_begin, group_end, cols)
    g, s = (np.empty(*o) for o in outs)
    _check(lib().mts_gram(*head, *mid, _ptr(g), _ptr(s), _ip(status)), 'mts_gram')
    return _status(status, n), g, s


def dev_gram(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, range_begin, range_end, window_rows, group_begin, group_end, cols,
             out=None, download=True):
    """mts_dev_gram on a DevBuffer of compressed chunks (offsets into it).  `out`: a DevBuffer for both results (Gram entries, then
    the sums at a 256-byte aligned offset; made when None, returned so that a caller timing repeated calls can pass it again).
    Returns (status list, gram or None, sum or None, out)."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, outs = _gram_args(dtype, range_begin, range_end, window_rows, group_begin, group_end, cols)
    out, ptrs, at = _dev_results(out, cbuf.device, [8 * int(np.prod(shape)) for shape, _ in outs])
    _check(lib().mts_dev_gram(*head, *mid, *ptrs, _ip(status)), 'mts_dev_gram')
    g, s = _dev_fetch(out, at, [np.empty(*o) for o in outs]) if download else (None, None)
    return _status(status, n), g, s, out


# -- the same Gram matrices over the filtered signal z of detect
def _fgram_args(valid_begin, valid_end, taps, cols, reference, range_begin, range_end, window_rows, group_begin, group_end):
    """-> (the op's own arguments of mts_filtered_gram, the shapes and dtypes of the Gram entries and the sums: float64, z is float32)."""
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).ravel())
    grid, outs = _gram_args(np.float32, range_begin, range_end, window_rows, group_begin, group_end, cols)
    mid = (int(valid_begin), int(valid_end), int(taps.size), _dp(taps)) + grid[5:7] + (int(reference),) + grid[:5]
    return mid, outs


def filtered_gram(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference,
                  range_begin, range_end, window_rows, group_begin, group_end, device=0):
    """mts_filtered_gram: the Gram entries and column sums of groups [group_begin, group_end) of the grid (range, window_rows) over z,
    the filtered rows of mts_detect (taps, cols, reference 0 / 1, float32 items), from the adjacent chunks `keys`, which cover the
    groups' filter support.  The grid and the summation tree are gram's for a float32 recording.  cache_id 0: no cache, every chunk
    comes with its bytes; else chunks with lens[i] == 0 must be resident (HipError E_MISS).  Returns (status list, gram (n_groups,
    n_cols, n_cols) float64, sum (n_groups, n_cols) float64), to be discarded when a status is not CHUNK_OK."""
    head, n, status = _host_chunks(device, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags)
    mid, outs = _fgram_args(valid_begin, valid_end, taps, cols, reference, range_begin, range_end, window_rows, group_begin, group_end)
    g, s = (np.empty(*o) for o in outs)
    _check(lib().mts_filtered_gram(*head, *mid, _dp(g), _dp(s), _ip(status)), 'mts_filtered_gram')
    return _status(status, n), g, s


def dev_filtered_gram(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags, valid_begin, valid_end, taps, cols, reference, range_begin,
                      range_end, window_rows, group_begin, group_end, out=None, download=True):
    """mts_dev_filtered_gram on a DevBuffer of compressed chunks (offsets into it).  `out`, download and the result as dev_gram."""
    head, n, status = _dev_chunks(cbuf, offs, lens, row0, n_rows, n_channels, dtype, flags)
    mid, outs = _fgram_args(valid_begin, valid_end, taps, cols, reference, range_begin, range_end, window_rows, group_begin, group_end)
    out, ptrs, at = _dev_results(out, cbuf.device, [8 * int(np.prod(shape)) for shape, _ in outs])
    _check(lib().mts_dev_filtered_gram(*head, *mid, *ptrs, _ip(status)), 'mts_dev_filtered_gram')
    g, s = _dev_fetch(out, at, [np.empty(*o) for o in outs]) if download else (None, None)
    return _status(status, n), g, s, out


# ------------------------------------------------------------------------------------------------
# device-resident recordings (bench.py, the tests at BASELINE's sizes): memory held through the library -- no second HIP runtime
# ------------------------------------------------------------------------------------------------
class HostBuffer:
    """Page-locked host memory (mts_host_alloc) as a numpy array: `.array` (uint8, nbytes).  Copies between it and the device are
    DMA transfers without a staging copy.  Keep the object alive while the array (or views of it) is in use."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _check(lib().mts_host_alloc(self.nbytes, C.byref(p)), 'mts_host_alloc')
        self.ptr = p.value or 0
        self.array = np.ctypeslib.as_array((C.c_ubyte * max(self.nbytes, 1)).from_address(self.ptr))[:self.nbytes]

    def free(self):
        if self.ptr:
            self.array = None
            ptr, self.ptr = self.ptr, 0
            _check(lib().mts_host_free(C.c_void_p(ptr)), 'mts_host_free')

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001
            pass


class PinnedPool:
    """Page-locked buffers kept between calls.  hipHostMalloc pins its pages one by one (a few hundred MB take a good part of a
    second) and hipHostFree unpins them again: a Reader.tofile that allocated its two piece buffers per call spent more time on
    that than on the file.  take() hands out an idle buffer of at least the size asked for (the smallest that fits, grown by
    a quarter when a new one has to be made); give() returns it; at most `keep_bytes` stay idle, the largest first
    (MTSCOMP_PINNED_KEEP_MB, default 2048; 0 keeps nothing).  clear() frees the idle ones: HipCodec.close() and release() call it."""

    def __init__(self, keep_bytes=None):
        import threading
        if keep_bytes is None:
            keep_bytes = int(os.environ.get('MTSCOMP_PINNED_KEEP_MB', 2048)) << 20
        self.keep_bytes = int(keep_bytes)
        self._idle = []
        self._lock = threading.Lock()

    def take(self, nbytes):
        nbytes = int(nbytes)
        with self._lock:
            fits = [b for b in self._idle if b.nbytes >= nbytes]
            if fits:
                best = min(fits, key=lambda b: b.nbytes)
                self._idle.remove(best)
                return best
        return HostBuffer(nbytes + nbytes // 4)

    def give(self, buf):
        if buf is None or not buf.ptr:
            return
        drop = []
        with self._lock:
            self._idle.append(buf)
            self._idle.sort(key=lambda b: -b.nbytes)
            while sum(b.nbytes for b in self._idle) > self.keep_bytes and len(self._idle) > 1:
                drop.append(self._idle.pop())
            if self._idle and (self._idle[0].nbytes > self.keep_bytes or self.keep_bytes <= 0):
                drop.append(self._idle.pop(0))
        for b in drop:
            b.free()

    def clear(self):
        with self._lock:
            idle, self._idle = self._idle, []
        for b in idle:
            b.free()


pinned_pool = PinnedPool()


def release():
    """Give back what the process keeps between calls: the idle page-locked buffers of `pinned_pool`, then the library's
    per-device workspaces (mts_release)."""
    pinned_pool.clear()
    if _lib is not None:
        _lib.mts_release()


class DevBuffer:
    """`nbytes` of HBM on `device`, allocated, copied and freed by libmtscomp_hip.so (mts_dev_alloc / mts_dev_copy / mts_dev_free)."""

    def __init__(self, nbytes, device=0):
        self.device, self.nbytes = int(device), int(nbytes)
        p = C.c_void_p()
        _check(lib().mts_dev_alloc(self.device, self.nbytes, C.byref(p)), 'mts_dev_alloc')
        self.ptr = p.value or 0

    def at(self, offset=0):
        assert 0 <= offset <= self.nbytes
        return C.c_void_p(self.ptr + int(offset))

    def upload(self, arr, offset=0):
        a = np.ascontiguousarray(arr)
        assert offset + a.nbytes <= self.nbytes
        _check(lib().mts_dev_copy(self.device, None, self.at(offset), _ptr(a), a.nbytes, 0), 'mts_dev_copy')

    def download(self, offset=0, nbytes=None, dtype=np.uint8):
        nbytes = self.nbytes - offset if nbytes is None else int(nbytes)
        assert offset + nbytes <= self.nbytes
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _check(lib().mts_dev_copy(self.device, None, _ptr(out), self.at(offset), out.nbytes, 1), 'mts_dev_copy')
        return out

    def diff(self, other, nbytes=None):
        """(bytes that differ, first such offset or -1) between this buffer and `other` (compared on the device)."""
        n, first = C.c_long(0), C.c_long(-1)
        nbytes = min(self.nbytes, other.nbytes) if nbytes is None else int(nbytes)
        _check(lib().mts_dev_compare(self.device, None, self.at(), other.at(), nbytes, C.byref(n), C.byref(first)), 'mts_dev_compare')
        return int(n.value), int(first.value)

    def free(self):
        if self.ptr:
            ptr, self.ptr = self.ptr, 0
            _check(lib().mts_dev_free(self.device, C.c_void_p(ptr)), 'mts_dev_free')

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def dev_sync(device=0):
    _check(lib().mts_dev_sync(int(device)), 'mts_dev_sync')


def dev_synth_int16(buf, offset, t0, t1, n_channels, seed=0):
    """Rows [t0, t1) of the synthetic recording written at `offset` of a DevBuffer."""
    assert offset + (t1 - t0) * n_channels * 2 <= buf.nbytes
    _check(lib().mts_dev_synth_int16(buf.device, None, buf.at(offset), int(t0), int(t1), int(n_channels), int(seed)), 'mts_dev_synth_int16')


def dev_compress_chunks(raw, n_channels, itemsize, bounds, flags, level, out, slots, sizes):
    """mts_dev_compress_chunks on DevBuffers: `bounds` rows (int64 array, n + 1), `slots` byte offsets into `out`, `sizes` filled."""
    _check(lib().mts_dev_compress_chunks(raw.device, None, raw.at(), n_channels, itemsize, _lp(bounds), len(bounds) - 1, int(flags), int(level),
                                         out.at(), _lp(slots), _lp(sizes)), 'mts_dev_compress_chunks')


def dev_decompress_chunks(cbuf, offs, lens, rows, n_channels, itemsize, flags, out, out_offs, status):
    """mts_dev_decompress_chunks on DevBuffers: chunk i is written at out_offs[i] of `out`, any multiple of the item size (HipError
    MTS_E_ARG otherwise); `status` (int32 array) is filled, a chunk that did not decode leaves its bytes of `out` as they were."""
    _check(lib().mts_dev_decompress_chunks(cbuf.device, None, cbuf.at(), _lp(offs), _lp(lens), _lp(rows), len(rows), n_channels, itemsize, int(flags),
                                           out.at(), _lp(out_offs), status.ctypes.data_as(C.POINTER(C.c_int))), 'mts_dev_decompress_chunks')


def last_stage_times(device=0):
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    n = lib().mts_last_stage_times(device, names, ms, 32)
    return [(names[i].decode(), float(ms[i])) for i in range(n)]


# ------------------------------------------------------------------------------------------------
# debug taps (GPU parity tests)
# ------------------------------------------------------------------------------------------------
def _u8(data):
    return np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8)) if not isinstance(data, np.ndarray) \
        else np.ascontiguousarray(data.view(np.uint8).ravel())


def debug_match_tables(data, level=6, device=0):
    a = _u8(data)
    tf = np.zeros(max(a.size, 1), dtype=np.uint32)
    tq = np.zeros(max(a.size, 1), dtype=np.uint32)
    _check(lib().mts_debug_match_tables(device, _ptr(a), a.size, level, _ptr(tf), _ptr(tq)), 'mts_debug_match_tables')
    return tf[:a.size], tq[:a.size]


def debug_tokens(data, level=6, device=0):
    a = _u8(data)
    toks = np.zeros((a.size + 1, 2), dtype=np.uint16)
    n = C.c_long(0)
    _check(lib().mts_debug_tokens(device, _ptr(a), a.size, level, _ptr(toks), C.byref(n)), 'mts_debug_tokens')
    return toks[:n.value].copy()


def debug_deflate(data, level=6, device=0):
    a = _u8(data)
    cap = compress_bound(a.size) + 64
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_long(0)
    _check(lib().mts_debug_deflate(device, _ptr(a), a.size, level, _ptr(out), cap, C.byref(n)), 'mts_debug_deflate')
    return out[:n.value].tobytes()


def debug_inflate(zbytes, expect_len, device=0):
    """Returns (status, bytes)."""
    z = _u8(zbytes)
    out = np.zeros(max(expect_len, 1), dtype=np.uint8)
    n, st = C.c_long(0), C.c_int(0)
    _check(lib().mts_debug_inflate(device, _ptr(z), z.size, _ptr(out), expect_len, C.byref(n), C.byref(st)),
           'mts_debug_inflate')
    return int(st.value), out[:n.value].tobytes()
