"""The block encoder (deflate.hip sections T, L, B: trees, layout, bit packing) and inflate's dynamic-header decoder on the
cases of tests/block_cases.py, at levels 1, 6 and 9: every edge of zlib's trees.c that tests/test_block_cases.py certifies the
cases to reach -- length-limited trees in all three alphabets, every kind of run item, HLIT / HDIST at both ends, stored
blocks at every bit phase, blocks that end with the token buffer, a block larger than the packer's image.

Bit-exact: the device's tokens are the oracle's, its bytes are zlib's, and zlib's bytes inflate to the data.  A failure names
the block the first wrong byte lies in and what that block holds.
"""
import numpy as np
import pytest

from mtscomp_amd import hip
from tests import block_cases as B
from tests import deflate_shape

pytestmark = pytest.mark.gpu
CASES = B.cases()
PAIRS = [(name, level) for name in CASES for level in B.LEVELS]
# the inflate test's other resolver and token paths: forced on the cases that overflow the distance tree and on gap(11)
ENV_CASES = [n for n in CASES if n.startswith('dist_stairs')] + ['gap_11']


def _first_diff(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    n = min(a.size, b.size)
    d = np.nonzero(a[:n] != b[:n])[0]
    return int(d[0]) if d.size else n


def _explain(name, level, got):
    """Where the device's stream leaves zlib's: byte, block, and what the block holds."""
    want = B.zbytes(name, level)
    at = _first_diff(got, want)
    i = deflate_shape.block_at(B.shape(name, level), at)
    where = B.describe_block(name, level, i) if i is not None else 'outside the blocks (zlib header or check value)'
    return '%s level %d: %d bytes for %d, first difference at byte %d (bit %d ..), %s' % (name, level, len(got), len(want), at, 8 * at, where)


@pytest.mark.parametrize('name,level', PAIRS)
def test_tokens(name, level):
    """The parse first: a different token is reported as one, not as a different tree."""
    want = B.oracle_report(name, level)[1]
    got = hip.debug_tokens(CASES[name], level)
    d = np.nonzero((got[:min(len(got), len(want))] != want[:min(len(got), len(want))]).any(axis=1))[0]
    assert got.shape == want.shape and not d.size, (got.shape, want.shape, int(d[0]) if d.size else None)


@pytest.mark.parametrize('name,level', PAIRS)
def test_deflate_bytes(name, level):
    got = hip.debug_deflate(CASES[name], level)
    assert got == B.zbytes(name, level), _explain(name, level, got)


def _inflate(name, level):
    data = CASES[name]
    st, out = hip.debug_inflate(B.zbytes(name, level), len(data))
    assert st == 0 and out == data, (name, level, st, len(out), _first_diff(out, data),
                                     [B.describe_block(name, level, i) for i in range(len(B.shape(name, level)))][:6])


@pytest.mark.parametrize('name,level', PAIRS)
def test_inflate(name, level):
    """zlib's stream through the device's decoder: 15-bit codes in both trees, 7-bit code-length codes, every run item, HLIT
    257 and 286, HDIST 30, stored blocks at every bit phase."""
    _inflate(name, level)


@pytest.mark.parametrize('env', [{'MTS_LZ_SEGS': '4'}, {'MTS_INF_NO_ROWS': '1'}], ids=['lz_segs_4', 'no_token_rows'])
@pytest.mark.parametrize('name', ENV_CASES)
def test_inflate_other_paths(monkeypatch, name, env):
    """The same streams with the LZ resolver cut into segments, and without pass A's token rows (pass B decodes every block)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for level in B.LEVELS:
        _inflate(name, level)


@pytest.mark.parametrize('level', B.LEVELS)
def test_batch_equals_one_at_a_time(level):
    """All cases as the chunks of ONE compress call and ONE decompress call (a byte stream is a one-channel uint8 recording
    without differences): the blocks of all chunks share the block kernels' grids in blk_chunk order, and a block's bytes must
    not depend on its neighbours.  (The empty stream is left out: a chunk has rows.)"""
    names = [n for n in CASES if len(CASES[n])]
    rows = [len(CASES[n]) for n in names]
    bounds = np.concatenate(([0], np.cumsum(rows)))
    x = np.frombuffer(b''.join(CASES[n] for n in names), dtype=np.uint8).reshape(-1, 1)
    got = hip.compress_chunks(x, bounds, 0, level)
    for n, z in zip(names, got):
        assert bytes(z) == B.zbytes(n, level), _explain(n, level, bytes(z))
    st, back = hip.decompress_chunks([B.zbytes(n, level) for n in names], rows, 1, 'uint8', 0)
    assert st == [0] * len(names), [(n, s) for n, s in zip(names, st) if s]
    for n, a in zip(names, back):
        assert a.tobytes() == CASES[n], (n, _first_diff(a.tobytes(), CASES[n]))
