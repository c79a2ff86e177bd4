"""K1, K2 and the adler32 summers of mtscomp_amd/csrc/transform.hip on the MI355X, on every tile height, alignment and batch of
tests/transform_cases.py (its CPU twin, tests/test_transform_cases.py, asserts which paths those cases reach).  The reference is the
reference's statement sequence on numpy (np.diff + tobytes(order), reshape + np.cumsum in the item's width) and, for the compressed
streams, stdlib zlib on it.  Bit-exact: no tolerance anywhere."""
import zlib

import numpy as np
import pytest

from mtscomp_amd import hip
from oracle import oracle as O
from tests import transform_cases as T

pytestmark = pytest.mark.gpu

CELLS = [(s, h) for s in (1, 2, 4) for h in T.HEIGHTS] + [(8, T.GENERIC)]
CELL_IDS = ['%dB-%s' % (s, h or 'generic') for s, h in CELLS]
E_ARG = -1


@pytest.fixture(scope='module', autouse=True)
def device():
    hip.require_device()


def _kernels(monkeypatch, generic):
    if generic:
        monkeypatch.setenv('MTS_K12_GENERIC', '1')
    else:
        monkeypatch.delenv('MTS_K12_GENERIC', raising=False)


def _check_single(x, flags, forced):
    """K1 and K2 on one chunk against the numpy reference; a wrong item is reported with its row, column, tile and path."""
    nt, nc = x.shape
    want = T.np_stream(x, flags)
    rows_kernels = flags == T.FLAGS_ROWS and not forced
    got = hip.delta_transpose(x, flags)
    if not np.array_equal(got, want):
        where = T.describe_k1(got, want, nt, nc, x.itemsize) if rows_kernels else int(np.nonzero(got != want)[0][0])
        pytest.fail('K1 %s %s flags %d%s: %s' % (x.dtype, x.shape, flags, ' (MTS_K12_GENERIC)' if forced else '', where))
    back = hip.cumsum_transpose(want, nt, nc, x.dtype, flags)
    assert back.dtype == x.dtype and back.shape == x.shape
    if back.tobytes() != x.tobytes():
        where = T.describe_k2(back, x, nt, nc, x.itemsize) if rows_kernels else np.argwhere(back != x)[0].tolist()
        pytest.fail('K2 %s %s flags %d%s: %s' % (x.dtype, x.shape, flags, ' (MTS_K12_GENERIC)' if forced else '', where))


# ---- single chunks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', T.FAMILIES)
@pytest.mark.parametrize('itemsize,height', CELLS, ids=CELL_IDS)
def test_single_chunk(itemsize, height, family, monkeypatch):
    """Every (width, row count, dtype) of the cell with the kernels its width gets, then with MTS_K12_GENERIC=1 (read on every launch)."""
    cases = [c for c in T.single_cases(itemsize, height) if c[2] == family]
    assert cases
    for forced in ((False, True) if height else (False,)):
        _kernels(monkeypatch, forced)
        for w, nt, fam, dt in cases:
            assert T.rows_tile(w, itemsize) == height
            _check_single(T.make(fam, dt, nt, w), T.FLAGS_ROWS, forced)


@pytest.mark.parametrize('family', T.FAMILIES)
@pytest.mark.parametrize('itemsize', [1, 2, 4, 8])
def test_generic_kernels_every_flag_set(itemsize, family, monkeypatch):
    """k_delta_transpose, k_spatial_cumsum, k_seg_sums and k_cumsum_transpose with all eight flag sets, around their 64-column tiles."""
    _kernels(monkeypatch, True)
    cases = [c for c in T.all_flags_cases(itemsize) if c[2] == family]
    assert cases
    for w, nt, fam, dt, flags in cases:
        _check_single(T.make(fam, dt, nt, w), flags, True)


# ---- K2 through the device entry: the caller's output offsets -------------------------------------------------------------------------
PATTERN_TAIL = 64


def _pattern(n):
    return ((np.arange(n, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)


class _Batch:
    """The chunks of a batch as zlib streams (level 1) in a DevBuffer, each at a multiple of 16 bytes, 16 spare bytes behind."""

    def __init__(self, w, rows, family, dtype, damage=None):
        self.w, self.rows, self.dtype = w, np.asarray(rows, np.int64), np.dtype(dtype)
        self.x, self.chunks = T.batch_data(w, rows, family, dtype)
        zs = [T.zstream(T.np_stream(c), 1) for c in self.chunks]
        for i, how in (damage or {}).items():
            z = bytearray(zs[i])
            z[{'trailer': len(z) - 1, 'body': len(z) // 2}[how]] ^= 0x55
            zs[i] = bytes(z)
        self.lens = np.array([len(z) for z in zs], np.int64)
        self.offs = np.concatenate(([0], np.cumsum((self.lens + 15) // 16 * 16)))[:-1].astype(np.int64)
        data = np.zeros(int(self.offs[-1] + self.lens[-1]) + 16, np.uint8)
        for o, z in zip(self.offs, zs):
            data[o:o + len(z)] = np.frombuffer(z, np.uint8)
        self.cbuf = hip.DevBuffer(data.size)
        self.cbuf.upload(data)
        self.sizes = self.rows * (w * self.dtype.itemsize)

    def decode(self, out, base, gap=0):
        """-> (status, the bytes of `out` after the call, the chunks' offsets): out filled with the pattern first, the chunks one
        after the other from `base` on, `gap` bytes between them."""
        n = len(self.rows)
        total = base + int(self.sizes.sum()) + (n - 1) * gap + PATTERN_TAIL
        assert total <= out.nbytes and out.ptr % 256 == 0
        ooffs = np.array(T.chunk_starts(self.rows, self.w, self.dtype.itemsize, base, gap), np.int64)
        out.upload(_pattern(total))
        status = np.full(len(self.rows), 99, np.int32)
        hip.dev_decompress_chunks(self.cbuf, self.offs, self.lens, self.rows, self.w, self.dtype.itemsize, T.FLAGS_ROWS, out, ooffs, status)
        return status, out.download(0, total), ooffs

    def free(self):
        self.cbuf.free()


def _check_decoded(b, status, got, ooffs, base, bad=()):
    """Every chunk's bytes are the reference's (a chunk in `bad`: untouched), every byte around and between them still holds the
    pattern."""
    pat = _pattern(got.size)
    outside = np.ones(got.size, bool)
    for i, c in enumerate(b.chunks):
        lo, hi = int(ooffs[i]), int(ooffs[i] + b.sizes[i])
        outside[lo:hi] = False
        if i in bad:
            assert status[i] != hip.CHUNK_OK, (i, status)
            assert np.array_equal(got[lo:hi], pat[lo:hi]), 'damaged chunk %d: its range was written' % i
            continue
        assert status[i] == hip.CHUNK_OK, (i, status)
        dec = np.frombuffer(got[lo:hi].tobytes(), b.dtype).reshape(c.shape)
        if dec.tobytes() != c.tobytes():
            pytest.fail('K2 %s width %d rows %s base %d, chunk %d: %s' % (b.dtype, b.w, b.rows.tolist(), base, i,
                                                                         T.describe_k2(dec, c, c.shape[0], b.w, b.dtype.itemsize, lo)))
    assert np.array_equal(got[:base], pat[:base]), 'bytes in front of the first chunk were written (base %d)' % base
    end = int(ooffs[-1] + b.sizes[-1])
    assert np.array_equal(got[end:], pat[end:]), 'bytes behind the last chunk were written'
    wrong = np.nonzero(outside & (got != pat))[0]
    assert not wrong.size, 'bytes between the chunks were written: %s (chunks at %s)' % (wrong[:8].tolist(), ooffs.tolist())


@pytest.fixture(scope='module')
def outbuf():
    buf = hip.DevBuffer(4 << 20)
    yield buf
    buf.free()


@pytest.mark.parametrize('itemsize,height', CELLS, ids=CELL_IDS)
def test_k2_dev_decompress_every_base(itemsize, height, outbuf):
    """Back-to-back output offsets, the whole output shifted by 0, one item, 4 and 16 bytes: each chunk starts at another alignment, so
    k_cumsum_rows takes its 16-byte, dword and item stores next to a neighbour's rows -- none of which may change.  Then the same
    with one item of pattern between the chunks: a store that runs over a chunk's end shows there, at every base."""
    for w, rows, fam, dt in T.batch_cases(itemsize, height):
        b = _Batch(w, rows, fam, dt)
        try:
            for gap in T.GAPS(itemsize):
                for base in T.BASES(itemsize):
                    status, got, ooffs = b.decode(outbuf, base, gap)
                    _check_decoded(b, status, got, ooffs, base)
        finally:
            b.free()


@pytest.mark.parametrize('how', ['trailer', 'body'])
@pytest.mark.parametrize('itemsize,height', CELLS, ids=CELL_IDS)
def test_k2_damaged_chunk_leaves_its_range(itemsize, height, how, outbuf):
    """A chunk whose compressed bytes are damaged (its check value, or a byte in the middle) keeps the pattern; its neighbours are right."""
    w = T.batch_widths(itemsize, height)[1]
    rows = T.batches(itemsize, height)[0]
    b = _Batch(w, rows, 'uniform', T.DTYPES[itemsize][0], damage={2: how})
    try:
        base = itemsize
        status, got, ooffs = b.decode(outbuf, base)
        _check_decoded(b, status, got, ooffs, base, bad=(2,))
        if how == 'trailer':
            assert status[2] == hip.CHUNK_CORRUPT
    finally:
        b.free()


@pytest.mark.parametrize('itemsize', [2, 4, 8])
def test_dev_decompress_refuses_a_misaligned_output(itemsize, outbuf):
    """d_out + out_offsets[i] must be a multiple of the item size: MTS_E_ARG naming the chunk, before anything is launched."""
    b = _Batch(65, [3, 5, 2], 'uniform', T.DTYPES[itemsize][0])
    try:
        total = int(b.sizes.sum()) + 64
        ooffs = np.concatenate(([0], np.cumsum(b.sizes)))[:-1].astype(np.int64)
        ooffs[1:] += itemsize // 2                                         # chunk 1 (and 2) off by half an item
        outbuf.upload(_pattern(total))
        status = np.full(3, 99, np.int32)
        with pytest.raises(hip.HipError) as e:
            hip.dev_decompress_chunks(b.cbuf, b.offs, b.lens, b.rows, b.w, itemsize, T.FLAGS_ROWS, outbuf, ooffs, status)
        assert e.value.code == E_ARG and 'chunk 1' in str(e.value) and 'multiple of the item size' in str(e.value)
        assert status.tolist() == [99, 99, 99] and np.array_equal(outbuf.download(0, total), _pattern(total))
        # any multiple of the item size is fine
        ooffs[1:] += itemsize - itemsize // 2
        hip.dev_decompress_chunks(b.cbuf, b.offs, b.lens, b.rows, b.w, itemsize, T.FLAGS_ROWS, outbuf, ooffs, status)
        assert status.tolist() == [0, 0, 0]
    finally:
        b.free()


# ---- K1 through the compressors: the trailer pins its adler32 sums ----------------------------------------------------------------------
def _check_streams(got, chunks, what):
    for i, (z, c) in enumerate(zip(got, chunks)):
        want = O.ref_compress_chunk(c, level=6)
        if z == want:
            continue
        stream = T.np_stream(c).tobytes()
        try:
            inflated = zlib.decompressobj(-15).decompress(z[2:])              # (the raw deflate data, no check value: what the encoder was given)
        except zlib.error as e:
            pytest.fail('%s chunk %d: not a deflate stream (%s): the encoder' % (what, i, e))
        if inflated != stream:
            where = T.describe_k1(np.frombuffer(inflated, np.uint8), np.frombuffer(stream, np.uint8), c.shape[0], c.shape[1], c.itemsize) \
                if len(inflated) == len(stream) else (len(inflated), len(stream))
            pytest.fail('%s chunk %d: K1 wrote a wrong stream: %s' % (what, i, where))
        if z[:-4] == want[:-4]:
            pytest.fail('%s chunk %d: the stream is right, the adler32 of K1 is not: %s, zlib %s' % (what, i, z[-4:].hex(), want[-4:].hex()))
        pytest.fail('%s chunk %d: K1 is right, the encoder differs from zlib' % (what, i))


@pytest.mark.parametrize('itemsize,height', CELLS, ids=CELL_IDS)
def test_k1_compress_batches(itemsize, height):
    """The batches at level 6 through mts_compress_chunks and mts_dev_compress_chunks: a chunk's rows start where the chunks before it
    end, so k_delta_rows takes its 16-byte and its item loads.  Every stream is zlib's, byte for byte, check value included."""
    for w, rows, fam, dt in T.batch_cases(itemsize, height):
        x, chunks = T.batch_data(w, rows, fam, dt)
        bounds = np.concatenate(([0], np.cumsum(rows))).astype(np.int64)
        what = '%s width %d rows %s %s' % (dt, w, rows, fam)
        _check_streams(hip.compress_chunks(x, bounds, T.FLAGS_ROWS, 6), chunks, 'compress_chunks ' + what)
        raw = hip.DevBuffer(x.nbytes + 256)
        caps = [(hip.compress_bound(c.nbytes) + 15) // 16 * 16 for c in chunks]
        slots = np.concatenate(([0], np.cumsum(caps)))[:-1].astype(np.int64)
        out = hip.DevBuffer(sum(caps) + 16)
        try:
            raw.upload(x)
            sizes = np.zeros(len(rows), np.int64)
            hip.dev_compress_chunks(raw, w, itemsize, bounds, T.FLAGS_ROWS, 6, out, slots, sizes)
            assert all(0 < s <= c for s, c in zip(sizes, caps))
            z = out.download()
            _check_streams([z[o:o + n].tobytes() for o, n in zip(slots, sizes)], chunks, 'dev_compress_chunks ' + what)
        finally:
            raw.free()
            out.free()


# ---- k_adler_stream (and the sums made in k_inf_translate) --------------------------------------------------------------------------------
@pytest.mark.parametrize('segs', [None, '1', '4'])
def test_adler_of_inflated_streams(segs, monkeypatch):
    """mts_debug_inflate verifies the check value with the device's sums: the stream must come back with status OK, and the same
    stream with a check value one too large must be CORRUPT.  MTS_LZ_SEGS=1: every byte summed by k_adler_stream; 4: a chunk cut
    into segments has its sums made where its bytes are (k_inf_translate); unset: the library's own choice."""
    if segs is None:
        monkeypatch.delenv('MTS_LZ_SEGS', raising=False)
    else:
        monkeypatch.setenv('MTS_LZ_SEGS', segs)
    for n in T.ADLER_SIZES:
        for name, data in T.adler_inputs(n):
            for level in T.ADLER_LEVELS:
                z = zlib.compress(data, level)
                st, out = hip.debug_inflate(z, n)
                assert st == hip.CHUNK_OK and out == data, (name, n, level, st)
                st, _ = hip.debug_inflate(T.bad_trailer(z), n)
                assert st == hip.CHUNK_CORRUPT, (name, n, level, st)
