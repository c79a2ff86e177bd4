"""The cases of tests/test_gpu_transform_edges.py (K1, K2 and the adler32 summers of mtscomp_amd/csrc/transform.hip on the MI355X) and of
their CPU twin tests/test_transform_cases.py: the launcher's decisions restated (which kernels a width gets, which branch a tile
takes), the value families, the widths, row counts and batches, and the references.  Plain Python and numpy: nothing here touches a
device.  Everything is bit-exact.

The restated decisions follow transform.hip line by line -- rows_pitch, rows_tile (and the constants beside it), the `if` in front of
the stream side of k_delta_rows / k_rows_sums / k_cumsum_rows, the load branches of k_delta_rows, the store branches of
k_cumsum_rows, the parts of k_rows_scan.  A change there is made here too; TRANSITIONS is asserted against rows_tile by the twin."""
import zlib

import numpy as np

from oracle import oracle as O

# ---- the launcher's decisions ------------------------------------------------------------------------------------------------------
ROWS_LDS_LIMIT = 64 * 1024           # what the launchers ask ensure_dynamic_lds for
ROWS_STATIC_LDS = 64                 # k_delta_rows: red[8] beside the dynamic image
ROWS_SCAN_PARTS = 8
FLAGS_ROWS = 5                       # time difference, channel-major stream: the only flags the row-tile kernels take
GENERIC = 0                          # tile "height" of the generic kernels


def rows_pitch(nc, itemsize):
    """LDS row pitch in items: at least nc, an odd number of dwords."""
    per = 4 // itemsize
    dw = (nc + per - 1) // per
    if not dw & 1:
        dw += 1
    return dw * per


def rows_tile(nc, itemsize):
    """Tile height of the row-tile kernels for a width (64, 32 or 16), or GENERIC: the generic kernels."""
    if itemsize > 4 or nc < 2:
        return GENERIC
    pitch_b = rows_pitch(nc, itemsize) * itemsize
    for tt in (64, 32, 16):
        if (tt + 1) * pitch_b + ROWS_STATIC_LDS <= ROWS_LDS_LIMIT:
            return tt
    return GENERIC


def delta_rows_lds(nc, itemsize):
    """Bytes of LDS of a k_delta_rows launch, static ones included (0: the width does not get that kernel)."""
    tt = rows_tile(nc, itemsize)
    return (tt + 1) * rows_pitch(nc, itemsize) * itemsize + ROWS_STATIC_LDS if tt else 0


def stream_fast(tt, nt, t0, itemsize, whole_tile_required):
    """The tile of rows [t0, t0 + tt) of a chunk of nt rows takes the 8-bytes-per-lane branch on the stream side.  K1 (k_delta_rows)
    takes it for a ragged last tile too; K2 (k_rows_sums, k_cumsum_rows) wants the tile whole.  (The stream of a chunk starts at a
    multiple of 256 bytes in the engine's workspace: the alignment term of the kernels' condition always holds.)"""
    ipl = 8 // itemsize
    ok = tt % ipl == 0 and (nt * itemsize) % 8 == 0 and (t0 * itemsize) % 8 == 0
    return ok and (not whole_tile_required or t0 + tt <= nt)


def store_path(addr, itemsize):
    """How k_cumsum_rows stores a tile whose first row lies at `addr`: 16 bytes per lane, whole dwords, or item by item."""
    assert addr % itemsize == 0 and itemsize <= 4
    return 'vec16' if addr % 16 == 0 else 'dword' if addr % 4 == 0 else 'item'


def load_path(addr):
    """How k_delta_rows loads a tile whose first row lies at `addr`."""
    return 'vec16' if addr % 16 == 0 else 'item'


def scan_parts(ntile):
    """k_rows_scan: the tiles [k_beg, k_end) of each of the ROWS_SCAN_PARTS parts of a chunk of ntile tiles."""
    per = (ntile + ROWS_SCAN_PARTS - 1) // ROWS_SCAN_PARTS
    out = []
    for part in range(ROWS_SCAN_PARTS):
        k_beg = min(part * per, ntile)
        out.append((k_beg, min(k_beg + per, ntile)))
    return out


def n_tiles(nt, tt):
    return (nt + tt - 1) // tt


# ---- widths -----------------------------------------------------------------------------------------------------------------------
# itemsize: the last width of tile heights 64, 32 and 16; the generic kernels start one above the last.  (Before rows_tile counted the
# static bytes of k_delta_rows, height 16 reached up to LDS_EDGE[itemsize][1]: a launch of 65 548 bytes against a limit of 65 536.)
TRANSITIONS = {1: (1004, 1980, 3844), 2: (502, 990, 1922), 4: (251, 495, 961)}
# the widths whose (16 + 1)-row image fits 64 KiB only without the static bytes, first and last: generic now
LDS_EDGE = {1: (3845, 3852), 2: (1923, 1926), 4: (962, 963)}
HEIGHTS = (64, 32, 16, GENERIC)
SMALL_WIDTHS = (2, 3, 63, 64, 65)
WIDTHS_8 = (1, 2, 63, 64, 65, 129)
ALL_FLAGS_WIDTHS = (63, 64, 65)       # every flag set on the generic kernels


def widths(itemsize):
    if itemsize == 8:
        return list(WIDTHS_8)
    w = set(SMALL_WIDTHS) | {385} | set(LDS_EDGE[itemsize]) | {LDS_EDGE[itemsize][1] + 1}
    for last in TRANSITIONS[itemsize]:
        w |= {last, last + 1}
    return sorted(w)


def widths_of(itemsize, height):
    return [w for w in widths(itemsize) if rows_tile(w, itemsize) == height]


def batch_widths(itemsize, height):
    """The narrowest and the widest width of a tile height (generic: the first generic width and the one behind the LDS edge)."""
    w = widths_of(itemsize, height)
    return [w[0], w[-1]]


# ---- row counts and batches ---------------------------------------------------------------------------------------------------------
def ipl_of(itemsize):
    return max(8 // itemsize, 1)


def row_counts(itemsize, height):
    tt, ipl = height or 64, ipl_of(itemsize)
    # (1, 2, 3 tiles; 8, 10 and 17 for k_rows_scan, and 7 * tt - 1 and 8 * tt + 1 for its 7 and 9)
    return [1, ipl + 1, tt - 1, tt, tt + 1, 2 * tt + ipl, 2 * tt + ipl + 1, 7 * tt - 1, 8 * tt, 8 * tt + 1, 9 * tt + 1, 17 * tt]


def batches(itemsize, height):
    """Lists of row counts for one call: mixed (every chunk start at another alignment), equal chunks, first longest and last one row."""
    tt, ipl = height or 64, ipl_of(itemsize)
    return [[tt + 1, 1, tt, 3, 2 * tt + ipl, 5], [2 * tt + ipl] * 3, [9 * tt + 1, tt, 1]]


def BASES(itemsize):
    """Shifts of the whole output of a K2 batch: none, one item, a dword, 16 bytes (those an item may lie at)."""
    return sorted(b for b in {0, itemsize, 4, 16} if b % itemsize == 0)


def GAPS(itemsize):
    """Unwritten bytes between the chunks of a K2 batch: none (back to back), and one item, so that a store that spills over a
    chunk's end is not hidden by the next chunk's own stores (and every chunk starts one item further off than back to back)."""
    return (0, itemsize)


def chunk_starts(rows, nc, itemsize, base=0, gap=0):
    """Byte address of every chunk of a batch laid out one after the other, `gap` bytes between (relative to a 16-byte aligned buffer)."""
    return [base + int(s) * nc * itemsize + i * gap for i, s in enumerate(np.concatenate(([0], np.cumsum(rows)[:-1])))]


# ---- values -----------------------------------------------------------------------------------------------------------------------
DTYPES = {1: ('int8', 'uint8'), 2: ('int16', 'uint16'), 4: ('int32', 'uint32'), 8: ('int64', 'uint64')}
FAMILIES = ('uniform', 'extremes', 'ff_stream')
_POOL = {}


def _pool(dtype, n):
    """Uniform random items over the full range of the dtype: one pool per dtype, cases are slices of it."""
    dtype = np.dtype(dtype)
    if dtype not in _POOL or _POOL[dtype].size < n:
        r = np.random.RandomState(1000 + dtype.num)
        size = max(n, 1 << 21)
        _POOL[dtype] = np.frombuffer(r.bytes(size * dtype.itemsize), dtype=dtype)
    return _POOL[dtype][:n]


def make(family, dtype, nt, nc):
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    if family == 'uniform':
        return _pool(dtype, nt * nc).reshape(nt, nc).copy()
    if family == 'extremes':
        # rows alternate min and max: every delta wraps, and the 64 deltas of a tile of 4-byte items (2^32 - 1 and 1 in turn) sum
        # past 2^32; the first, middle and last column are constant (all their deltas but the first are zero)
        x = np.empty((nt, nc), dtype=dtype)
        x[0::2], x[1::2] = info.min, info.max
        for c, v in ((0, info.max), (nc // 2, info.min), (nc - 1, 1)):
            x[:, c] = v
        return x
    if family == 'ff_stream':
        # x[t, c] = -(t + 1) in the item width: the first row and every difference are -1, every byte of the stream is 0xff
        u = np.dtype('u%d' % dtype.itemsize)
        col = (np.zeros(nt, dtype=u) - (np.arange(nt, dtype=np.uint64) + np.uint64(1)).astype(u)).view(dtype)
        return np.repeat(col[:, None], nc, axis=1)
    raise ValueError(family)


# ---- references: the reference's statement sequence on numpy ------------------------------------------------------------------------
def np_stream(x, flags=FLAGS_ROWS):
    """K1: diff_along_axis (time, then space) + tobytes(order), as the reference's writer does."""
    d = O.ref_diff_along_axis(x, axis=0 if flags & 1 else None)
    d = O.ref_diff_along_axis(d, axis=1 if flags & 2 else None)
    return np.frombuffer(d.tobytes(order='F' if flags & 4 else 'C'), dtype=np.uint8)


def np_unstream(stream, nt, nc, dtype, flags=FLAGS_ROWS):
    """K2: reshape(order) + cumsum (space, then time) in the item's own width + ascontiguousarray, as the reference's reader does."""
    dtype = np.dtype(dtype)
    c = np.frombuffer(bytes(stream), dtype=dtype).reshape((nt, nc), order='F' if flags & 4 else 'C')
    if flags & 2:
        c = np.cumsum(c, axis=1, dtype=dtype)
    if flags & 1:
        c = np.cumsum(c, axis=0, dtype=dtype)
    return np.ascontiguousarray(c)


def single_cases(itemsize, height):
    """(width, rows, family, dtype) of every single-chunk case of a (itemsize, tile height) cell."""
    return [(w, nt, fam, dt) for w in widths_of(itemsize, height) for nt in row_counts(itemsize, height) for fam in FAMILIES
            for dt in DTYPES[itemsize]]


def all_flags_cases(itemsize):
    """(width, rows, family, dtype, flags) of the generic kernels' cases with all eight flag sets: the widths around their 64-column
    tiles (the 8-byte widths for 8-byte items), whatever kernels those widths get otherwise."""
    return [(w, nt, fam, dt, fl) for w in (WIDTHS_8 if itemsize == 8 else ALL_FLAGS_WIDTHS) for nt in row_counts(itemsize, GENERIC)
            for fam in FAMILIES for dt in DTYPES[itemsize] for fl in range(8)]


def batch_cases(itemsize, height):
    """(width, row counts, family, dtype) of every batch of a cell.  ff_stream at the widest width only (its chunks are all alike)."""
    out = []
    for k, w in enumerate(batch_widths(itemsize, height)):
        for rows in batches(itemsize, height):
            for fam in FAMILIES:
                if fam == 'ff_stream' and k == 0:
                    continue
                out += [(w, rows, fam, dt) for dt in DTYPES[itemsize]]
    return out


def batch_data(w, rows, family, dtype):
    """-> (the batch's rows as one array, its chunks)."""
    x = make(family, dtype, int(sum(rows)), w)
    b = np.concatenate(([0], np.cumsum(rows)))
    return x, [x[b[i]:b[i + 1]] for i in range(len(rows))]


# ---- where a wrong item lies --------------------------------------------------------------------------------------------------------
def describe_k1(got, want, nt, nc, itemsize, raw_addr=0):
    """The first item of a channel-major stream (uint8 arrays) that differs, as (row, column, tile, path)."""
    u = np.dtype('u%d' % itemsize)
    d = np.nonzero(got.view(u) != want.view(u))[0]
    if not d.size:
        return None
    t, c = int(d[0]) % nt, int(d[0]) // nt
    tt = rows_tile(nc, itemsize)
    if not tt:
        return dict(row=t, col=c, tile=(t // 64, c // 64), path='generic', n_wrong=int(d.size))
    t0 = t // tt * tt
    path = 'stream %s, load %s' % ('8 B per lane' if stream_fast(tt, nt, t0, itemsize, False) else 'item',
                                   load_path(raw_addr + t0 * nc * itemsize))
    return dict(row=t, col=c, tile=t // tt, path=path, n_wrong=int(d.size))


def describe_k2(got, want, nt, nc, itemsize, out_addr=0):
    """The first item of a decoded (nt, nc) chunk that differs, as (row, column, tile, path)."""
    u = np.dtype('u%d' % itemsize)
    d = np.nonzero(np.ascontiguousarray(got).view(u).ravel() != np.ascontiguousarray(want).view(u).ravel())[0]
    if not d.size:
        return None
    t, c = int(d[0]) // nc, int(d[0]) % nc
    tt = rows_tile(nc, itemsize)
    if not tt:
        return dict(row=t, col=c, tile=(t // 64, c // 64), path='generic', n_wrong=int(d.size))
    t0 = t // tt * tt
    path = 'stream %s, store %s' % ('8 B per lane' if stream_fast(tt, nt, t0, itemsize, True) else 'item',
                                    store_path(out_addr + t0 * nc * itemsize, itemsize))
    return dict(row=t, col=c, tile=t // tt, path=path, n_wrong=int(d.size))


# ---- adler32 ----------------------------------------------------------------------------------------------------------------------
# the 16-byte step of k_adler_stream and its scalar tail, a workgroup's 16 KiB share, sums that pass 65521 many times over
ADLER_SIZES = (1, 15, 16, 17, 31, 16383, 16384, 16385, 65536, 65537, 1048576 + 5)
ADLER_LEVELS = (0, 6)


def adler_inputs(n):
    """(name, bytes): nothing but 0xff -- the largest A and B -- and random bytes of the same length."""
    return [('ff', b'\xff' * n), ('random', np.random.RandomState(n % 65521).bytes(n))]


def bad_trailer(z):
    """A zlib stream with a check value one above the right one."""
    a = (int.from_bytes(z[-4:], 'big') + 1) & 0xffffffff
    return z[:-4] + a.to_bytes(4, 'big')


def zstream(stream, level=1):
    return zlib.compress(bytes(stream), level)
