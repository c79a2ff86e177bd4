"""inflate.hip on the catalogue of tests/inflate_cases.py: streams that are valid deflate but that zlib's encoder never writes,
and streams that zlib refuses (tests/test_inflate_cases.py certifies on the CPU that zlib and the oracle give the verdict each
case claims and that each limit-seeking case crosses its limit).

Every case alone through mts_debug_inflate; the catalogue again under every other path of the decoder (the block-after-block
decoder alone, pass B without token rows, no row pool, the segmented resolver, the resolver's retry pass); the whole catalogue
as the chunks of one decompress_chunks call with a refused stream on both sides of every valid one; and, for the cases that
overflow a capacity limit of the fast path, proof that the fallback ran: the wave decoder took longer than for a zlib stream of
the same output size -- and, for the cases that stay inside a limit or have another way round it, that it did not.
"""
import time
import zlib

import numpy as np
import pytest

from mtscomp_amd import hip
from tests import deflate_shape
from tests import inflate_cases as I
from tests import inputs

pytestmark = pytest.mark.gpu
CAT = I.catalogue()
SMALL = [n for n in CAT if not CAT[n].large]
# the limits whose overflow hands the chunk to the wave decoder (k_inf_wave).  Not among them: the cases that stay just inside a
# limit, 'rowcap' (pass B decodes the block again) and 'chain_lds_cand' (the chain walks its candidates from memory instead of LDS)
FALLBACK = ('subcap_over', 'true_cap', 'cand_cap', 'inline_over', 'final_zone', 'wave_round')
OTHER_PATHS = [{'MTS_INFLATE_SEQ': '1'}, {'MTS_INF_NO_ROWS': '1'}, {'MTS_INF_ROW_ROUNDS': '0'}, {'MTS_LZ_SEGS': '2'}, {'MTS_LZ_SEGS': '4'},
               {'MTS_LZ_FORCE_RETRY': '1', 'MTS_LZ_SEGS': '1'}, {'MTS_LZ_FORCE_RETRY': '1', 'MTS_LZ_SEGS': '4'}]


@pytest.fixture(scope='module', autouse=True)
def warm():
    st, out = hip.debug_inflate(zlib.compress(b'code objects and workspaces'), 27)          # (not on a case's clock)
    assert st == 0


def _first_diff(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    n = min(a.size, b.size)
    d = np.nonzero(a[:n] != b[:n])[0]
    return int(d[0]) if d.size else n


def _where(name, at):
    """The block that output byte `at` of a case comes from, and where that block lies in the stream."""
    c = CAT[name]
    if c.block_out is None:
        return 'a stream zlib wrote'
    blks = deflate_shape.blocks(c.z_shape)
    ends = np.cumsum(c.block_out)
    i = min(int(np.searchsorted(ends, at, side='right')), len(blks) - 1)
    b = blks[i]
    first = b['bit_start'] // 8
    return 'block %d of %d (type %d, stream bits %d .. %d, output bytes %d .. %d; stream byte %d belongs to block %s)' % (
        i, len(blks), b['btype'], b['bit_start'], b['bit_end'], int(ends[i]) - c.block_out[i], int(ends[i]), first, deflate_shape.block_at(blks, first))


def _verdict(name, st, out, dt=None):
    """None, or what is wrong with the device's answer to a case."""
    c = CAT[name]
    if c.data is None:
        if st != hip.CHUNK_CORRUPT:
            return '%s: zlib refuses the stream, the device says %d' % (name, st)
        if dt is not None and dt >= 2.0:
            return '%s: refused after %.1f s' % (name, dt)
        return None
    if st != 0:
        return '%s: a valid stream of %d bytes for %d, the device says %d' % (name, len(c.stream), c.n, st)
    if out != c.data:
        at = _first_diff(out, c.data)
        return '%s: %d bytes for %d, first difference at byte %d, %s' % (name, len(out), c.n, at, _where(name, at))
    return None


def _run(name):
    c = CAT[name]
    t0 = time.perf_counter()
    st, out = hip.debug_inflate(c.stream, c.n)
    return _verdict(name, st, out, time.perf_counter() - t0)


@pytest.mark.parametrize('name', list(CAT))
def test_case(name):
    """Valid: status 0 and the bytes.  Refused: CHUNK_CORRUPT within the 2.0 s of test_inflate_errors."""
    bad = _run(name)
    assert bad is None, bad


@pytest.mark.parametrize('name', I.SIZE_CASES)
def test_wrong_size_and_wrong_check(name):
    """A valid stream of another length is a size mismatch; with a damaged check value it is corrupt whatever its length (the
    order test_inflate_errors fixes: the check value is looked at before the size, as zlib.decompress does)."""
    c = CAT[name]
    for n in (c.n - 1, c.n + 1):
        st, _ = hip.debug_inflate(c.stream, n)
        assert st == hip.CHUNK_BADSIZE, (name, n, st)
    z = I.wrong_check(c.stream)
    for n in (c.n - 1, c.n, c.n + 1):
        st, _ = hip.debug_inflate(z, n)
        assert st == hip.CHUNK_CORRUPT, (name, n, st)


@pytest.mark.parametrize('env', OTHER_PATHS, ids=['+'.join('%s=%s' % kv for kv in e.items()) for e in OTHER_PATHS])
def test_other_paths(monkeypatch, env):
    """The catalogue (without the three large cases, which add nothing here) with every chunk through the block-after-block
    decoder, with pass B decoding every block, without a row pool, with the resolver cut into 2 and 4 segments -- the pair
    'distance_101_...' is the same distance refused in the first segment and legal in a later one -- and through the retry pass."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bad = [b for b in (_run(name) for name in SMALL) if b]
    assert not bad, '%d of %d: %s' % (len(bad), len(SMALL), '; '.join(bad[:8]))


@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_catalogue_as_one_batch(order):
    """Every case that produces bytes as one chunk of ONE decompress_chunks call (a byte stream is a one-channel uint8 recording
    without differences; a chunk has rows, so the empty-output cases are left out): a refused stream on both sides of every
    valid one, one status per chunk, the valid chunks' bytes untouched by their neighbours."""
    valid = [n for n in CAT if CAT[n].data]
    refused = [n for n in CAT if CAT[n].data is None]
    names = []
    for k, n in enumerate(valid):
        names += [refused[k % len(refused)], n]
    names.append(refused[len(valid) % len(refused)])
    if order == 'reversed':
        names.reverse()
    st, arrs = hip.decompress_chunks([CAT[n].stream for n in names], [CAT[n].n for n in names], 1, 'uint8', 0)
    assert len(st) == len(names)
    bad = [b for b in (_verdict(n, s, a.tobytes() if a is not None else b'') for n, s, a in zip(names, st, arrs)) if b]
    assert not bad, '%d of %d: %s' % (len(bad), len(names), '; '.join(bad[:8]))


def _wave_ms(z, n):
    st, out = hip.debug_inflate(z, n)
    return st, out, dict(hip.last_stage_times())['inflate_wave_decoder']


@pytest.fixture(scope='module')
def filler():
    return inputs.textlike(4500000, 77)


@pytest.mark.parametrize('name', [n for n in CAT if CAT[n].limit in FALLBACK])
def test_the_fallback_ran(name, filler):
    """A case that overflows a limit of the fast path is finished by the wave decoder: its stage takes longer than for a zlib
    level-6 stream of the same output size decoded just before it (which leaves the wave decoder nothing to do)."""
    c = CAT[name]
    plain = filler[:c.n]
    st, out, base = _wave_ms(zlib.compress(plain, 6), c.n)
    assert st == 0 and out == plain
    st, out, ms = _wave_ms(c.stream, c.n)
    assert _verdict(name, st, out) is None
    assert ms > base, (name, c.limit, base, ms)


@pytest.mark.parametrize('name', [n for n in CAT if CAT[n].limit and CAT[n].limit not in FALLBACK])
def test_the_fast_path_kept_it(monkeypatch, name):
    """The cases that stay inside a limit, or cross one that has its own way round (pass A starting again with full-length
    sub-sequences, pass B decoding a block whose rows overflowed, the chain walking its candidates from memory), leave the wave
    decoder nothing to do.  Compared with the same stream under MTS_INFLATE_SEQ, where the wave decoder does all of it: less than
    half.  (Half separates an empty launch from decoding the chunk's one large block, which is most of the chunk; without pass A's
    second start the block with headers in its bits takes the wave decoder as long as the whole chunk does.)"""
    c = CAT[name]
    st, out, ms = _wave_ms(c.stream, c.n)
    assert _verdict(name, st, out) is None
    monkeypatch.setenv('MTS_INFLATE_SEQ', '1')
    st, out, ms_seq = _wave_ms(c.stream, c.n)
    assert _verdict(name, st, out) is None
    assert 2 * ms < ms_seq, (name, c.limit, ms, ms_seq)


@pytest.mark.parametrize('under,over', [('dynamic_block_just_under_511_subsequences', 'dynamic_block_just_over_511_subsequences'),
                                        ('fixed_block_of_4096_bytes_after_a_dynamic_block', 'fixed_block_of_4097_bytes_after_a_dynamic_block')])
def test_the_limit_lies_between_the_pair(under, over):
    """The two streams differ by one token: the one inside the limit leaves the wave decoder less to do than the one past it."""
    a, b = CAT[under], CAT[over]
    st, out, ms_under = _wave_ms(a.stream, a.n)
    assert _verdict(under, st, out) is None
    st, out, ms_over = _wave_ms(b.stream, b.n)
    assert _verdict(over, st, out) is None
    assert ms_over > ms_under, (ms_under, ms_over)
