"""The match finder (match.hip: k_match5 for levels 4..6, k_match6 for 7..9) and the lazy parse (deflate.hip) on the cases of
tests/match_cases.py: every off-by-one rule of zlib's longest_match / deflate_slow and every boundary of the kernels' geometry
that tests/test_match_cases.py certifies the cases to reach -- chain budget and quarter budget, hash runs across 64-slot groups,
wave and workgroup starts, 15-bit hash collisions, the 7- and 13-byte limits of the compare, nice_match, MAX_DIST for the chain
head and for the rest, position 0, good_match / max_lazy / TOO_FAR in the parse, the end of a chunk, the tile seam, chunks back
to back.

Bit-exact: the device's tables are the oracle's, its tokens are the oracle's, its bytes are zlib's.  A failure names the first
wrong position, where the kernel has it (tile, slot, group, lane), both results, and how the reference walk went there.
"""
import numpy as np
import pytest

from mtscomp_amd import hip
from oracle import oracle as O
from tests import match_cases as M

pytestmark = pytest.mark.gpu
CASES = M.cases()
PAIRS = M.pairs()
SLICE_LEVELS = (4, 5, 6)


def _check_tables(name, level, what=''):
    data = CASES[name].data
    tf, tq = O.match_tables(data, level)
    gf, gq = hip.debug_match_tables(data, level)
    for label, got, want in (('t_full', gf, tf), ('t_quarter', gq, tq)):
        d = np.nonzero(got != want)[0]
        if d.size:
            p = int(d[0])
            raise AssertionError('%s%s: %d wrong, first: device (len %d, dist %d), oracle (len %d, dist %d); %s' % (
                what, label, d.size, int(got[p]) >> 16, int(got[p]) & 0xffff, int(want[p]) >> 16, int(want[p]) & 0xffff,
                M.explain(name, level, p)))


@pytest.mark.parametrize('name,level', PAIRS)
def test_match_tables(name, level):
    _check_tables(name, level)


@pytest.mark.parametrize('env', ['1', '64'])
@pytest.mark.parametrize('name', [n for n, c in CASES.items() if set(c.levels) & set(SLICE_LEVELS)])
def test_match_tables_other_slices(monkeypatch, name, env):
    """k_match5 with one workgroup per tile (a wave walks many groups and carries its ring along) and with 64 (on these small
    streams: one group per wave, every group stages its history again)."""
    monkeypatch.setenv('MTS_MATCH_SLICES', env)
    for level in SLICE_LEVELS:
        if level in CASES[name].levels:
            _check_tables(name, level, 'MTS_MATCH_SLICES=%s, ' % env)


@pytest.mark.parametrize('name,level', PAIRS)
def test_tokens(name, level):
    data = CASES[name].data
    _, want, pos, _ = O.deflate(data, level, report=True)
    got = hip.debug_tokens(data, level)
    k = min(len(got), len(want))
    d = np.nonzero((got[:k] != want[:k]).any(axis=1))[0]
    if d.size or got.shape != want.shape:
        i = int(d[0]) if d.size else k
        p = int(pos[min(i, len(pos) - 1)])
        raise AssertionError('%d tokens for %d, first wrong: token %d, device %s, oracle %s; %s' % (
            len(got), len(want), i, got[i].tolist() if i < len(got) else None, want[i].tolist() if i < len(want) else None,
            M.explain(name, level, p)))


@pytest.mark.parametrize('name', list(CASES))
def test_deflate_bytes(name):
    """zlib's bytes at every level the case claims, and at the fast levels 1..3 for every case."""
    data = CASES[name].data
    for level in (1, 2, 3) + tuple(CASES[name].levels):
        got = hip.debug_deflate(data, level)
        want = M.zbytes(name, level)
        assert got == want, (name, level, len(got), len(want), int(np.argmax(np.frombuffer(got, np.uint8)[:min(len(got), len(want))] !=
                                                                             np.frombuffer(want, np.uint8)[:min(len(got), len(want))])))


@pytest.mark.parametrize('level', [6, 9])
def test_batch_equals_one_at_a_time(level):
    """All cases as the chunks of ONE compress call: tiles of many chunks share the match kernels' grids, and a chunk's tables
    must not depend on its neighbours in the stream buffer."""
    names = list(CASES)
    rows = [len(CASES[n].data) for n in names]
    bounds = np.concatenate(([0], np.cumsum(rows)))
    x = np.frombuffer(b''.join(CASES[n].data for n in names), dtype=np.uint8).reshape(-1, 1)
    got = hip.compress_chunks(x, bounds, 0, level)
    bad = [n for n, z in zip(names, got) if bytes(z) != M.zbytes(n, level)]
    assert not bad, bad


@pytest.mark.parametrize('level', [1, 4, 6, 9])
def test_chunks_back_to_back(level):
    """One periodic stream cut at arbitrary phases: a chunk's matches neither reach back into the chunk before it nor go on
    into the one behind it -- each chunk is zlib's of that chunk alone."""
    import zlib
    data = M.chunked_stream()
    cuts = np.asarray(M.CHUNK_CUTS)
    x = np.frombuffer(data, dtype=np.uint8).reshape(-1, 1)
    got = hip.compress_chunks(x, cuts, 0, level)
    for i, z in enumerate(got):
        assert bytes(z) == zlib.compress(data[cuts[i]:cuts[i + 1]], level), (level, i, int(cuts[i]), int(cuts[i + 1]))
