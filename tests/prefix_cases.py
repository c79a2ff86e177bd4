"""Chunks for the leading-channel prefix decode (mts_cache_read_slices_leading), device-free: arrays, their compressed streams from
several writers, and for each stream the table of its deflate blocks -- where every block ends in the stream's bits and how many
bytes of output have been produced by then.  tests/test_prefix_cases.py certifies the catalogue on the CPU (zlib, the oracle's
transforms); tests/test_gpu_prefix_reads.py and tools/fuzz_prefix_reads_gpu.py run it through the device.

For k leading channels of a chunk of R rows:

    n_need          R * k * itemsize: the prefix of the (channel-major) stream that holds them
    covering block  the first block whose cumulative output reaches n_need
    L_min           the byte that holds the covering block's last bit: ceil(bit_end / 8)

A CLASS names where n_need falls (CLASSES below); the certification asserts that every class is reached by some (case, k).
"""
import functools
import zlib

import numpy as np

from oracle import oracle as O
from tests import deflate_build as D
from tests.deflate_shape import blocks

NC = 130
K_INT16 = (1, 2, 3, 16, 63, 64, 65, 129)     # 1: the generic kernel; 2 and up: the row tile; 63 / 64 / 65: a wave; 129: n_channels - 1
K_OTHER = (1, 3, 65)
ROWS_INT16 = (0, 1, 2, 63, 1999, 2000)
FLAGS = tuple(O.make_flags(td, sd, 'F') for td in (True, False) for sd in (False, True))
CHAIN_INLINE_BYTES = 4096                   # inflate.hip: the longest unannounced Huffman block the chain walk counts itself
CLASSES = ('first', 'middle', 'final', 'exact', 'stored', 'fixed_short', 'fixed_long', 'dynamic', 'empty_stored_near', 'no_rows')


def signal(dtype, rows, seed, nc=NC, const_lead=0):
    """Noise around a slow sine (channels compress about equally); the first const_lead channels constant."""
    dtype = np.dtype(dtype)
    rs = np.random.RandomState(seed)
    amp = {1: 6., 2: 900., 4: 4.e6, 8: 4.e6}[dtype.itemsize]
    x = rs.randn(rows, nc) * amp + rs.randn(nc) * 3 * amp + 2 * amp * np.sin(np.arange(rows) / 300.)[:, None]
    if dtype.kind == 'u':
        x += 128
    info = np.iinfo(dtype)
    x = x.clip(info.min, info.max).astype(dtype)
    if const_lead and rows:
        x[:, :const_lead] = x[0, :const_lead]
    return x


def table(z):
    """[(bit_end, cumulative nout, btype, nout, last)] per block of the zlib stream z."""
    out, cum = [], 0
    for b in blocks(z):
        cum += b['nout']
        out.append((b['bit_end'], cum, b['btype'], b['nout'], b['last']))
    return out


class Case:
    def __init__(self, name, arr, flags, z, ks, writer):
        self.name, self.arr, self.flags, self.z, self.ks, self.writer = name, arr, flags, bytes(z), tuple(ks), writer
        self.table = table(self.z)
        self.rows, self.nc = arr.shape
        self.dtype = arr.dtype

    def n_need(self, k):
        return self.rows * k * self.dtype.itemsize

    def cover(self, k):
        need = self.n_need(k)
        return next(i for i, t in enumerate(self.table) if t[1] >= need)

    def l_min(self, k):
        return (self.table[self.cover(k)][0] + 7) // 8

    def classes(self, k):
        t, i, need = self.table, self.cover(k), self.n_need(k)
        c = set()
        if self.rows == 0:
            return {'no_rows'}
        c.add('exact' if t[i][1] == need else 'final' if t[i][4] else 'first' if i == 0 else 'middle')
        c.add(('stored', 'fixed_short' if t[i][3] < CHAIN_INLINE_BYTES else 'fixed_long', 'dynamic')[t[i][2]])
        if any(0 <= j < len(t) and t[j][2] == 0 and t[j][3] == 0 for j in (i - 1, i + 1)):
            c.add('empty_stored_near')
        return c

    def lengths(self, k):
        """The sweep of S1: 24 evenly spaced lengths from 2 to len(z), L_min - 2 .. L_min + 2, len(z) - 5 .. len(z)."""
        n, lm = len(self.z), self.l_min(k)
        ls = set(int(x) for x in np.linspace(2, n, 24)) | {lm + d for d in range(-2, 3)} | {n - d for d in range(6)}
        return sorted(x for x in ls if 2 <= x <= n)

    def __repr__(self):
        return self.name


def stream_of(arr, flags):
    return bytes(O.delta_transpose(arr, flags)) if arr.size else b''


def zlib_stream(stream, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, cut=None, flush=zlib.Z_SYNC_FLUSH):
    """stdlib zlib's bytes; cut: flush (an empty stored block) after that many bytes of input."""
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    if cut is None:
        return c.compress(stream) + c.flush()
    return c.compress(stream[:cut]) + c.flush(flush) + c.compress(stream[cut:]) + c.flush()


def written(stream, plan):
    """tests/deflate_build.Writer: the stream cut into blocks, plan = [(type 0 | 1 | 2, bytes)], literals only; the last block is final
    and takes what is left."""
    w, at = D.Writer(), 0
    for j, (kind, n) in enumerate(plan):
        final = j == len(plan) - 1
        part = stream[at:] if final else stream[at:at + n]
        at += len(part)
        if kind == 0:
            w.stored(part, final)
        elif kind == 1:
            w.fixed([part], final)
        else:
            w.dynamic([part], final)
    assert at == len(stream)
    z = D.zwrap(w, stream)
    # the writer's own record of its blocks is what the stream reader finds (block_bits count from the first deflate bit)
    assert [(t[0] - 16, t[3]) for t in table(z)] == [(b[2], n) for b, n in zip(w.block_bits, w.block_out)]
    return z, w


def _plan_around(need, kind, size, before, total, piece=12000):
    """Dynamic blocks of `piece` bytes, then a block of `kind` and `size` bytes that starts `before` bytes ahead of `need`, then
    dynamic blocks again."""
    plan, at = [], 0
    start = max(need - before, 0)
    while at + piece <= start:
        plan.append((2, piece))
        at += piece
    if start > at:
        plan.append((2, start - at))
        at = start
    plan.append((kind, size))
    at += size
    while at < total:
        plan.append((2, min(piece, total - at)))
        at += piece
    return plan


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, arr, flags, z, ks, writer):
        out.append(Case(name, arr, flags, z, ks, writer))

    td = FLAGS[0]
    a16 = signal('int16', 2000, 1)
    for f in FLAGS:                                                   # every flag combination, every leading count
        add('i16_2000_f%d_l6' % f, a16, f, zlib_stream(stream_of(a16, f)), K_INT16, 'zlib6')
    s16 = stream_of(a16, td)
    add('i16_2000_l1', a16, td, zlib_stream(s16, 1), (1, 16, 65), 'zlib1')
    add('i16_2000_l9', a16, td, zlib_stream(s16, 9), (1, 16, 65), 'zlib9')
    add('i16_2000_fixed', a16, td, zlib_stream(s16, 6, zlib.Z_FIXED), (1, 65), 'fixed')
    add('i16_2000_stored', a16, td, zlib_stream(s16, 0), (1, 3, 65), 'stored')
    for k in (16, 65):
        need = 2000 * k * 2
        for d in (-1, 0, 1):
            add('i16_2000_sync%+d_k%d' % (d, k), a16, td, zlib_stream(s16, 6, cut=need + d), (k,), 'sync')
        add('i16_2000_full_k%d' % k, a16, td, zlib_stream(s16, 6, cut=need, flush=zlib.Z_FULL_FLUSH), (k,), 'full')
    for rows in ROWS_INT16[:-1]:                                      # chunks of 0 / 1 / 2 / 63 rows, and 1999 (rows not 8-byte aligned)
        a = signal('int16', rows, 2 + rows)
        for f in (FLAGS[0], FLAGS[1]):
            add('i16_%d_f%d_l6' % (rows, f), a, f, zlib_stream(stream_of(a, f)), K_INT16, 'zlib6')
    for dt in ('uint8', 'int32', 'int64'):
        a = signal(dt, 2000, 7)
        for f in FLAGS:
            add('%s_2000_f%d_l6' % (dt, f), a, f, zlib_stream(stream_of(a, f)), K_OTHER, 'zlib6')
    ac = signal('int16', 2000, 9, const_lead=65)                      # the leading channels are a few hundred bytes of the stream
    add('i16_2000_const65_l6', ac, td, zlib_stream(stream_of(ac, td)), (1, 64, 65), 'zlib6')
    add('i16_2000_const65_f%d_l6' % FLAGS[1], ac, FLAGS[1], zlib_stream(stream_of(ac, FLAGS[1])), (1, 65), 'zlib6')
    # hand-built streams (literals only): what no encoder writes at a chosen place
    a63 = signal('int16', 63, 11)
    z, _ = written(stream_of(a63, td), [(2, 0)])
    add('i16_63_one_dynamic_block', a63, td, z, (1, 3, 65, 129), 'writer')
    a500 = signal('int16', 500, 12)
    s500 = stream_of(a500, td)
    for k in (16, 65):
        need = 500 * k * 2
        for what, kind, size, before in (('stored', 0, 3000, 1000), ('fixed_short', 1, 2000, 1000), ('fixed_long', 1, 8000, 3000)):
            z, _ = written(s500, _plan_around(need, kind, size, before, len(s500)))
            add('i16_500_%s_k%d' % (what, k), a500, td, z, (k,), 'writer')
        z, _ = written(s500, _plan_around(need, 2, 5000, 5000, len(s500)))
        add('i16_500_exact_k%d' % k, a500, td, z, (k,), 'writer')
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def pairs(writers=None):
    return [(c, k) for c in cases() for k in c.ks if writers is None or c.writer in writers]


@functools.lru_cache(maxsize=None)
def poison(dtype, rows, nc=NC):
    """Another chunk of the same shape (its zlib level 6 stream, default flags): decoded whole before a prefix call, it leaves the
    engine's stream and token buffers full of plausible wrong bytes."""
    a = signal(dtype, rows, 1234)
    a = (a[::-1] ^ 0x55).astype(a.dtype)
    return zlib.compress(stream_of(a, FLAGS[0]), 6)


def expected(case, k):
    return np.ascontiguousarray(case.arr[:, :k])


def prefix_inverse(case, k):
    """arr[:, :k] from the first n_need bytes of the stream, by the oracle's inverse transform."""
    need = case.n_need(k)
    return O.cumsum_transpose(np.frombuffer(zlib.decompress(case.z)[:need], dtype=np.uint8), case.rows, k, case.dtype, case.flags)
