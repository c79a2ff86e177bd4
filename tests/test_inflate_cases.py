"""The catalogue of tests/inflate_cases.py certified on the CPU: zlib.decompress gives the verdict and the bytes each case
claims, the oracle's inflate gives the same, deflate_shape.blocks() finds the blocks each case was built to have, and every
case that aims at a capacity limit of inflate.hip (the constants are quoted in inflate_cases.py) is shown to cross it -- a case
that misses its limit fails here, not silently on the GPU.  Then the unit tests of the stream writer, tests/deflate_build.py.
"""
import time
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import deflate_build as D
from tests import deflate_shape
from tests import inflate_cases as I
from tests import inputs

CAT = I.catalogue()
VALID = [n for n, c in CAT.items() if c.data is not None]
REFUSED = [n for n, c in CAT.items() if c.data is None]


@pytest.fixture(scope='module')
def shapes():
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = deflate_shape.blocks(CAT[name].z_shape)
        return memo[name]
    return get


def test_the_catalogue_builds_quickly_and_the_same_twice():
    """Linear builder: the whole catalogue, its three large cases included, in a few seconds; seeded: the same bytes again."""
    I.catalogue.cache_clear()
    t0 = time.perf_counter()
    again = I.catalogue()
    dt = time.perf_counter() - t0
    assert dt < 10.0, dt
    assert list(again) == list(CAT)
    assert all(again[n].stream == CAT[n].stream and again[n].data == CAT[n].data for n in CAT)
    assert sorted(n for n in CAT if CAT[n].large) == ['1100_tiny_dynamic_blocks_in_stored_filler', 'dynamic_block_of_three_times_511_subsequences',
                                                        'final_block_starts_before_the_final_zone']
    assert I.cases().keys() == CAT.keys() and len(VALID) > 60 and len(REFUSED) > 35


def test_a_4_mb_stream_builds_in_about_a_second():
    w = D.Writer()
    filler = bytes(60000)
    lits = I.rnd(20000, 1, 200)
    t0 = time.perf_counter()
    for k in range(60):
        w.stored(filler, False)
        w.dynamic([lits, (258, 32768)], False)
    w.fixed([], True)
    z = D.zwrap(w)
    dt = time.perf_counter() - t0
    assert len(z) > 4000000 and dt < 3.0, (len(z), dt)
    assert zlib.decompress(z) == D.expand(w.tokens)


@pytest.mark.parametrize('name', VALID)
def test_zlib_and_the_oracle_accept(name):
    c = CAT[name]
    assert zlib.decompress(c.stream) == c.data
    got, used = O.inflate(c.stream, len(c.data))
    assert got == c.data
    assert used == len(c.z_shape)                       # (the oracle stops behind the check value)


@pytest.mark.parametrize('name', REFUSED)
def test_zlib_and_the_oracle_refuse(name):
    c = CAT[name]
    with pytest.raises(zlib.error):
        zlib.decompress(c.stream)
    with pytest.raises(ValueError):
        O.inflate(c.stream, c.n + 1000)
    assert c.n >= 1


@pytest.mark.parametrize('name', VALID)
def test_block_structure(name, shapes):
    c = CAT[name]
    blks = shapes(name)
    got = [(b['btype'], b['len'] if b['btype'] == 0 else b['ntok']) for b in blks]
    if c.shape is None:                                  # zlib's own stream: what it is in the catalogue for
        assert name == 'zlib_partial_flush'
        assert sum(1 for b in blks if b['btype'] == 1 and b['ntok'] == 0 and not b['last']) >= 6
        return
    assert got == c.shape
    assert [b['last'] for b in blks] == [0] * (len(blks) - 1) + [1]
    assert [(b['bit_start'] - 16, b['bit_end'] - 16) for b in blks] == [(p[0], p[2]) for p in c.block_bits]
    assert sum(c.block_out) == len(c.data)


def _dyn_headers(blks):
    return [b for b in blks if b['btype'] == 2]


def test_the_edges_the_cases_name(shapes):
    """What the names promise, read back from the streams."""
    pads = [b['pad'] for b in shapes('stored_at_every_bit_phase') if b['btype'] == 0]
    assert sorted(pads) == list(range(8))
    blks = shapes('block_types_alternate_at_every_bit_phase')
    for t in (0, 1, 2):
        assert {b['bit_start'] % 8 for b in blks if b['btype'] == t} == set(range(8)), t
    for name, hlit, hdist, hclen in (('hlit257_hdist1_hclen5', 257, 1, 5), ('hlit286_hdist30_hclen19', 286, 30, 19)):
        b = [b for b in _dyn_headers(shapes(name)) if (b['hlit'], b['hdist'], b['hclen']) == (hlit, hdist, hclen)]
        assert len(b) == 2, name
    for b in shapes('header_of_316_explicit_lengths'):
        assert b['items'] == [] and b['hlit'] + b['hdist'] == 316
    for name in ('codes_of_8_9_15_bits_eob_all_ones', 'codes_of_8_9_15_bits_length_all_ones', 'hlit286_hdist30_hclen19'):
        assert all(b['l_max_len'] == 15 and b['d_max_len'] == 15 for b in _dyn_headers(shapes(name))[-2:]), name
    b = _dyn_headers(shapes('only_code_is_a_1_bit_end_of_block'))
    assert [(x['l_max_len'], x['d_max_len'], x['ntok']) for x in b if x['ntok'] == 0] == [(1, 0, 0)] * 3
    assert [x['d_max_len'] for x in shapes('one_distance_code_used')] == [1, 1]
    assert [x['d_max_len'] for x in shapes('no_distance_code_literals_only')] == [0, 0]
    assert (16, 6) in shapes('item_16_carries_a_length_into_the_distance_lengths')[0]['items']
    assert (18, 14) in shapes('item_18_spans_both_alphabets')[0]['items']
    assert shapes('stored_len_65535')[0]['len'] == 65535
    for name in ('text', 'ar1'):
        n = CAT['deflate_stream_in_stored_blocks_%s' % name].n
        assert 90000 < n < 130000 and CAT['deflate_stream_as_fixed_literals_%s' % name].n == n
        assert len(deflate_shape.blocks(CAT['deflate_stream_in_stored_blocks_%s' % name].data)) >= 3     # (the payload has blocks of its own)


def _survivors(z):
    """Bit offsets of the stream that pass the scan's filters (block type 2, HLIT and HDIST <= 29, a complete code-length code,
    100 bits of stream behind them): every candidate the validator can announce is among them."""
    bits = np.unpackbits(np.frombuffer(z, np.uint8), bitorder='little')
    n = bits.size - I.SCAN_MIN_BITS + 1
    if n <= 16:
        return []
    b = lambda j: bits[j:j + n].astype(bool)
    m = ~b(1) & b(2) & ~(b(4) & b(5) & b(6) & b(7)) & ~(b(9) & b(10) & b(11) & b(12))
    m[:16] = False
    out = []
    for o in np.nonzero(m)[0]:
        o = int(o)
        hclen = int(bits[o + 13:o + 17] @ (1, 2, 4, 8)) + 4
        f = bits[o + 17:o + 17 + 3 * hclen].reshape(-1, 3) @ (1, 2, 4)
        if sum(128 >> int(l) for l in f if l) == 128:
            out.append(o)
    return out


LIMIT_CASES = [n for n, c in CAT.items() if c.limit]


def test_every_limit_has_a_case():
    assert {CAT[n].limit for n in LIMIT_CASES} == set(I.LIMITS)


@pytest.mark.parametrize('name', LIMIT_CASES)
def test_limit_is_crossed(name, shapes):
    c = CAT[name]
    z, blks = c.stream, shapes(name)
    dyn = _dyn_headers(blks)
    announced = [b for b in dyn if b['bit_start'] + I.SCAN_MIN_BITS <= 8 * len(z)
                 and (not b['last'] or 8 * len(z) - b['bit_start'] < 8 * I.SCAN_FINAL_ZONE)]
    full = (I.SUBCAP - 1) * I.SUB_BITS
    if c.limit == 'subcap_under':
        # flat 8-bit codes: the end-of-block code starts (body_bits - 8) // 1024 sub-sequences in, and 511 can be recorded
        big = max(b['body_bits'] for b in dyn)
        assert full - 64 < big <= full and (big - 8) // I.SUB_BITS + 1 == I.SUBCAP - 1
    elif c.limit == 'subcap_over':
        big = max(b['body_bits'] for b in dyn)
        assert big > full and (big - 8) // I.SUB_BITS + 1 > I.SUBCAP - 1
        if name.endswith('just_over_511_subsequences'):
            assert big == full + 8
    elif c.limit == 'true_cap':
        assert len(blks) > I.true_cap(len(z)) and len(z) < 2048
    elif c.limit == 'cand_cap':
        assert len(announced) > I.cand_cap(len(z)) and len(z) < 2048 + 512
    elif c.limit == 'chain_lds_cand':
        assert len(announced) > I.CHAIN_LDS_CAND
        assert len(_survivors(z)) < I.cand_cap(len(z))            # (all of them fit: the chain walk sees every candidate)
        assert len(blks) < I.true_cap(len(z))
    elif c.limit in ('inline_at', 'inline_over'):
        k = [i for i, b in enumerate(blks) if b['btype'] == 1]
        assert len(k) == 1 and blks[k[0] - 1]['btype'] == 2 and not blks[k[0]]['last']
        assert c.block_out[k[0]] == I.CHAIN_INLINE_BYTES + (c.limit == 'inline_over')
    elif c.limit == 'final_zone':
        last = blks[-1]
        assert last['btype'] == 2 and last['last'] and last['ntok'] > 0
        assert 8 * len(z) - last['bit_start'] > 8 * I.SCAN_FINAL_ZONE + 2 * 32768        # (two scan spans to spare)
    elif c.limit == 'wave_round':
        assert max(b['body_bits'] for b in blks if b['btype'] == 1) > I.WAVE_ROUND_BITS
    elif c.limit == 'rowcap':
        b = max(dyn, key=lambda b: b['ntok'])
        subs = -(-b['body_bits'] // I.SUB_BITS)
        assert 33 * (b['ntok'] // subs) > I.ROWCAP                 # 258 bytes at distance 1: 33 pieces of 8 bytes a token
    elif c.limit == 'subcap_retry':
        # the first block of the inner stream, bit for bit in the body (no 9-bit literal before its header ends): a candidate
        # 16 bits behind the header of the block that holds it, so that block is cut into sub-sequences of SUB_MIN bits ...
        big = max(dyn, key=lambda b: b['body_bits'])
        body0 = big['bit_end'] - big['body_bits']
        inner = bytes(I.rev8(v) for v in c.data[200:200 + big['ntok']])
        first = deflate_shape.blocks(inner)[0]
        hdr_end = 16 + 3 + first['hdr_bits']
        assert first['btype'] == 2 and not first['last'] and 255 not in inner[:hdr_end // 8 + 1]
        bits = np.unpackbits(np.frombuffer(z, np.uint8), bitorder='little')
        ibits = np.unpackbits(np.frombuffer(inner, np.uint8), bitorder='little')
        assert np.array_equal(bits[body0 + 16:body0 + hdr_end], ibits[16:hdr_end])
        assert body0 + 16 in _survivors(z)
        # ... of which 511 do not reach its end, while 511 of full length do
        assert (I.SUBCAP - 1) * I.SUB_MIN + 64 * 48 < big['body_bits'] <= full
    else:
        raise AssertionError(c.limit)


def test_size_cases_are_valid_cases():
    for name in I.SIZE_CASES:
        c = CAT[name]
        assert c.data is not None and c.n >= 1
        with pytest.raises(zlib.error):
            zlib.decompress(I.wrong_check(c.stream))


# ---- the writer ---------------------------------------------------------------------------------------------------------
FREQS = {
    'skewed': [int(1.6 ** i) + 1 for i in range(40)],                  # Huffman's tree is ~28 deep
    'fibonacci': [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765],
    'flat': [7] * 286,
    'flat_power_of_two': [1] * 128,
    'single': [0] * 9 + [5] + [0] * 20,
    'none': [0] * 30,
    'two': [0, 3, 0, 1],
    'sparse': [0, 900, 0, 0, 1, 0, 17, 0, 0, 0, 2, 1, 1, 250],
}


@pytest.mark.parametrize('maxbits', [7, 9, 15])
@pytest.mark.parametrize('what', list(FREQS))
def test_limited_lengths(what, maxbits):
    f = FREQS[what]
    if sum(1 for x in f if x) > 1 << maxbits:
        with pytest.raises(ValueError):
            D.limited_lengths(f, maxbits)
        return
    lens = D.limited_lengths(f, maxbits)
    assert len(lens) == len(f) and max(lens) <= maxbits
    assert sum(2.0 ** -l for l in lens if l) == 1.0                   # complete
    assert all(l > 0 for l, x in zip(lens, f) if x)
    assert sum(1 for l in lens if l) == max(2, sum(1 for x in f if x))
    codes = D.canonical(lens)                                          # a prefix code
    words = sorted(format(c, '0%db' % l) for c, l in zip(codes, lens) if l)
    assert all(not b.startswith(a) for a, b in zip(words, words[1:]))
    used = [(x, l) for x, l in zip(f, lens) if x]                      # never a longer code for a more frequent symbol
    assert all(la <= lb for (xa, la) in used for (xb, lb) in used if xa > xb)


def _tokens_of(z):
    """The tokens, trees and header items of the ONE dynamic block of the zlib stream `z` (decoded with deflate_shape's reader)."""
    S = deflate_shape
    blks = S.blocks(z)
    assert len(blks) == 1 and blks[0]['btype'] == 2
    b = blks[0]
    bits = S._Bits(z[:-4], 16 + 3 + 14)
    bits.take(3 * b['hclen'])
    dec = S._decoder(b['bl_lens'])
    lens, items = [], []
    while len(lens) < b['hlit'] + b['hdist']:
        s = S._sym(bits, dec)
        if s < 16:
            lens.append(s)
            items.append(s)
        else:
            rep = bits.take((2, 3, 7)[s - 16]) + (3, 3, 11)[s - 16]
            lens += [lens[-1] if s == 16 else 0] * rep
            items.append((s, rep))
    ll, dl = lens[:b['hlit']], lens[b['hlit']:]
    ldec, ddec = S._decoder(ll), S._decoder(dl)
    toks = []
    while True:
        s = S._sym(bits, ldec)
        if s == 256:
            break
        if s < 256:
            toks.append(s)
            continue
        ln = D.LEN_BASE[s - 257] + bits.take(D.LEN_EXTRA[s - 257])
        d = S._sym(bits, ddec)
        toks.append((ln, D.DIST_BASE[d] + bits.take(D.DIST_EXTRA[d])))
    return toks, ll, dl, items, b


@pytest.mark.parametrize('what', ['text', 'ar1', 'runs'])
def test_canonical_agrees_with_zlib(what):
    """A stream zlib wrote, taken apart and written again by the builder with zlib's own lengths, counts and items: the same
    bytes, so the codes the builder derives from the lengths are zlib's (and its bit order, its extra bits, its header)."""
    data = {'text': inputs.textlike(6000, 3), 'ar1': inputs.ar1_stream(200, 8), 'runs': bytes(700) + inputs.repeats(5000, 4)}[what]
    z = zlib.compress(data, 6)
    toks, ll, dl, items, b = _tokens_of(z)
    assert D.expand(toks) == data
    w = D.Writer()
    w.dynamic(toks, True, lit_lens=ll, dist_lens=dl, hlit=b['hlit'], hdist=b['hdist'], hclen=b['hclen'], cl_items=items, cl_lens=b['bl_lens'])
    assert D.zwrap(w, flg=z[1]) == z
    assert D.run_items(ll + dl) == items or D.expand(w.tokens) == data      # (the greedy items need not be zlib's)


def test_writer_bits_and_fields():
    w = D.Writer()
    w.bits(0b101, 3)
    w.code(0b110, 3)                                     # a Huffman code goes first bit first: 1, 1, 0
    w.bits(0x1ff, 9)
    assert w.bitpos == 15 and w.getvalue() == bytes([0b11011101, 0b01111111])
    w.align()
    w.raw_bytes(b'xy')
    assert w.getvalue() == bytes([0b11011101, 0b01111111]) + b'xy' and w.bitpos == 32
    assert D.canonical([2, 1, 3, 3]) == [0b10, 0b0, 0b110, 0b111]                        # RFC 1951, 3.2.2
    assert D.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]
    assert [D.dist_sym(d) for d in (1, 4, 5, 6, 7, 24576, 24577, 32768)] == [0, 3, 4, 4, 5, 28, 29, 29]
    assert D.expand([1, 2, 3, (7, 3), b'ab', (3, 1)]) == bytes([1, 2, 3, 1, 2, 3, 1, 2, 3, 1]) + b'abbbb'
    with pytest.raises(ValueError):
        D.expand([1, (3, 2)])
    for cmf in (0x08, 0x78, 0x88):
        for fl in range(4):
            assert ((cmf << 8) | D.flg_for(cmf, fl)) % 31 == 0 and D.flg_for(cmf, fl) >> 6 == fl
    assert D.zwrap(b'\x03\x00', b'')[:2] == b'\x78\x9c' and zlib.decompress(D.zwrap(b'\x03\x00', b'')) == b''
