"""The one-pass hash sort's scatter (k_op_scatter: one returning LDS atomic per key, the rank kept in a register) and the block
packer's bit positions (k_block_pack: a wave's first bit from the range totals k_block_trees leaves with the block) at the
smallest shapes that reach their edges.  Every case is one small chunk, fed as a ready-made stream; the device's bytes must be
stdlib zlib's.

Scatter: a tile is sorted in one pass only with at least 2 x 8192 keys and at most 1024 live hash buckets; a slice is 8192 keys
(16 waves x 8 instructions x 64 lanes), a bucket's per-wave counter a 16-bit half of a word it shares with its neighbour.  A
wrong rank would not show in the bytes -- the match stage sees a hash run out of order and the tile is sorted again by the
ballot ranking -- so every case also asserts that no such second sort ran.

Packer: a wave owns 2048 token indices of the block's 16384 (16383 tokens and the end-of-block code, which has index ntok).
test_cases_are_what_they_are_named_for checks on the CPU that zlib's own stream for every case has the block type and token
count its name says, and the scatter inputs the tiles, keys and buckets.
"""
import functools
import zlib

import numpy as np
import pytest

from mtscomp_amd import hip
from tests import block_cases as B
from tests import deflate_shape

LEVELS = (1, 6, 9)
TILE, HALO, SLICE, LMAX = 229376, 32768, 8192, 1024      # codec_plan.h: TILE, HALO; deflate.hip: OP_SLICE, OP_LMAX
IMG_BITS = 32 * 8192                                     # deflate.hip: PACK_IMG_WORDS


# ------------------------------------------------------------------------------------------------
# scatter
# ------------------------------------------------------------------------------------------------
def _alphabet(n, nsym, seed):
    return np.random.RandomState(seed).randint(0, nsym, size=n).astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def sort_cases():
    return {
        'one_bucket': b'\x07' * 20000,                                       # every wave's 512 keys on one half-word
        'two_buckets_one_word': b'ab' * 10000,                               # both halves of one counter word busy
        'last_slice_37_keys': _alphabet(3 * SLICE + 39, 8, 11),              # lanes past the end take no rank
        '1000_buckets_9_slices': _alphabet(70000, 10, 12),                   # the offsets across slices
        'second_tile_with_halo': _alphabet(TILE + 20000, 6, 13),
    }


def tiles_of(n):
    """(window start, hashed positions) of every tile of a stream of n bytes (codec_plan.h: CompressPlan)."""
    out = []
    for a in range(0, max(n, 1), TILE):
        w = max(0, a - HALO)
        out.append((w, max(0, min(a + TILE, n - 2) - w)))
    return out


def live_buckets(data, w, wlen):
    """Distinct zlib hashes of the positions [w, w + wlen)."""
    d = np.frombuffer(data, np.uint8).astype(np.uint32)
    h = ((d[w:w + wlen] << 10) ^ (d[w + 1:w + wlen + 1] << 5) ^ d[w + 2:w + wlen + 2]) & 0x7fff
    return np.unique(h)


def _check_sort_case(name):
    data = sort_cases()[name]
    tiles = tiles_of(len(data))
    for w, wlen in tiles:
        live = live_buckets(data, w, wlen)
        assert wlen >= 2 * SLICE and live.size <= LMAX, (name, w, wlen, live.size)      # the one-pass path
    return tiles


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(sort_cases()))
def test_scatter_bytes_and_no_resort(name):
    _check_sort_case(name)
    data = sort_cases()[name]
    got = hip.debug_deflate(data, 6)
    stages = [n for n, _ in hip.last_stage_times(0)]
    assert got == zlib.compress(data, 6), (name, len(got))
    assert 'hash_sort' in stages and 'hash_sort_retry' not in stages, stages


# ------------------------------------------------------------------------------------------------
# packer
# ------------------------------------------------------------------------------------------------
TOKENS = (1, 63, 64, 65, 2047, 2048, 2049, 4096, 16383)


def skewed_literals(n, nsym, seed):
    """n bytes of `nsym` symbols with weights 1.6 ** -i, a byte skipped when it would complete a trigram seen before: n literal
    tokens and no match, few enough symbols that even 63 of them are worth a code (block_cases.literal_only's 200 symbols are
    stored at that size)."""
    r = np.random.RandomState(seed)
    p = 1.6 ** -np.arange(nsym)
    p /= p.sum()
    out, seen = bytearray(), set()
    while len(out) < n:
        for b in r.choice(nsym, size=256, p=p):
            t = (out[-2], out[-1], int(b)) if len(out) >= 2 else None
            if t is not None and t in seen:
                continue
            seen.add(t)
            out.append(int(b))
            if len(out) == n:
                break
    return bytes(out)


@functools.lru_cache(maxsize=None)
def pack_cases():
    """name -> (bytes, {level: (block index, btype, tokens, larger than the image)}): what zlib makes of the stream, certified by
    test_cases_are_what_they_are_named_for."""
    c = {}
    every = lambda *e: {lv: e for lv in LEVELS}
    c['literals_1_fixed'] = (b'\x5a', every(0, 1, 1, False))
    for n in (63, 64, 65):
        c['literals_%d_dynamic' % n] = (skewed_literals(n, 9, 300 + n), every(0, 2, n, False))
    for n in (2047, 2048, 2049, 4096, 16383):
        c['literals_%d_dynamic' % n] = (B.literal_only(n, 100 + n), every(0, 2, n, False))
    for n in (63, 64, 65):                              # 8 words: 32 literals, the rest matches of 4 bytes
        c['mixed_%d_fixed' % n] = (B.all_matches(n, seed=n, nwords=8), every(0, 1, n, False))
    for n in (2047, 2048, 2049, 4096, 16383):           # 160 words: 640 literals
        c['mixed_%d_dynamic' % n] = (B.all_matches(n, seed=n), every(0, 2, n, False))
    # copies from 16 .. 32 KiB back: distance codes 28 and 29, 13 extra bits each.  A part of a block, and a full block that is
    # larger than the packer's image at levels 6 and 9 (level 1 finds fewer of the copies: its block fits)
    c['far_copies_part_block'] = (B.short_farcopies(2, 3000), {1: (2, 2, 3537, False), 6: (2, 2, 3484, False), 9: (2, 2, 3484, False)})
    c['far_copies_past_the_image'] = (B.short_farcopies(1), {1: (2, 2, 16383, False), 6: (2, 2, 16383, True), 9: (2, 2, 16383, True)})
    return c


@functools.lru_cache(maxsize=None)
def _zbytes(name, level):
    return zlib.compress(pack_cases()[name][0], level)


@pytest.mark.gpu
@pytest.mark.parametrize('level', LEVELS)
@pytest.mark.parametrize('name', list(pack_cases()))
def test_pack_bytes(name, level):
    data = pack_cases()[name][0]
    got, want = hip.debug_deflate(data, level), _zbytes(name, level)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        n = min(a.size, b.size)
        d = np.nonzero(a[:n] != b[:n])[0]
        at = int(d[0]) if d.size else n
        blks = deflate_shape.blocks(want)
        i = deflate_shape.block_at(blks, at)
        where = 'outside the blocks' if i is None else 'block %d (btype %d, %s tokens, bits [%d, %d))' % (
            i, blks[i]['btype'], blks[i].get('ntok'), blks[i]['bit_start'], blks[i]['bit_end'])
        pytest.fail('%s level %d: %d bytes for %d, first difference at byte %d (bit %d ..), %s' % (name, level, len(got), len(want), at, 8 * at, where))


# ------------------------------------------------------------------------------------------------
# the cases themselves, on the CPU
# ------------------------------------------------------------------------------------------------
def test_cases_are_what_they_are_named_for(monkeypatch):
    assert all(any(k.startswith(p + '_%d_' % n) for k in pack_cases()) for n in TOKENS for p in ('literals', 'mixed') if (p, n) != ('mixed', 1))
    took13 = [0]
    take = deflate_shape._Bits.take

    def counting_take(self, k):                          # (nothing but a distance code's extra bits is 13 bits long)
        took13[0] += k == 13
        return take(self, k)
    monkeypatch.setattr(deflate_shape._Bits, 'take', counting_take)
    seen = set()
    for name, (data, expect) in pack_cases().items():
        for level in LEVELS:
            took13[0] = 0
            blks = deflate_shape.blocks(_zbytes(name, level))
            i, btype, ntok, past = expect[level]
            b = blks[i]
            assert (b['btype'], b['ntok']) == (btype, ntok), (name, level, [(x['btype'], x.get('ntok')) for x in blks])
            assert all(x['btype'] == 0 for x in blks[:i]), (name, level)               # the first block with tokens
            assert (b['bit_end'] - (b['bit_start'] & ~31) > IMG_BITS) == past, (name, level, b['bit_start'], b['bit_end'])
            if name.startswith('far_copies'):
                assert took13[0] > ntok // 2, (name, level, took13[0])
            if name.startswith('literals'):
                assert btype != 2 or b['hdist'] <= 2, (name, level, b['hdist'])          # no distance code in use (zlib forces two)
            seen.add((btype, past))
    assert seen == {(1, False), (2, False), (2, True)}
    # the scatter inputs: every tile on the one-pass path, and the edge each is named for
    t = {n: _check_sort_case(n) for n in sort_cases()}
    s = sort_cases()
    assert [live_buckets(s['one_bucket'], *t['one_bucket'][0]).size, live_buckets(s['two_buckets_one_word'], *t['two_buckets_one_word'][0]).size] == [1, 2]
    assert t['last_slice_37_keys'][0][1] % SLICE == 37
    assert live_buckets(s['1000_buckets_9_slices'], *t['1000_buckets_9_slices'][0]).size == 1000 and -(-t['1000_buckets_9_slices'][0][1] // SLICE) == 9
    assert len(t['second_tile_with_halo']) == 2 and t['second_tile_with_halo'][1][0] == TILE - HALO
