"""The catalogue of hand-built zlib streams that inflate.hip is held to: streams that are valid RFC 1950 / 1951 but that zlib's
encoder never writes, and streams that zlib.decompress refuses.  Built with tests/deflate_build.py, seeded and deterministic.

    cases()      name -> (stream, data or None)      None: zlib refuses the stream
    catalogue()  name -> Case                        the same with what the tests need to know about a case

tests/test_inflate_cases.py certifies every entry on the CPU (zlib, the oracle, the block structure, the limits a case aims
at); tests/test_gpu_inflate_streams.py runs every entry through the device.

To add a case: write a function below that builds the stream with a Writer, hand it to C.ok() (expected bytes come from
expand() of the writer's tokens) or C.bad() (state how many bytes the caller would expect), and, if the case aims at a
capacity limit of the decoder, give `limit=` a key of LIMITS so that the CPU test proves the stream crosses it.
"""
import functools
import zlib

import numpy as np

from tests import deflate_build as D
from tests import inputs

# the capacity limits of inflate.hip's fast path, quoted from the code (mtscomp_amd/csrc/inflate.hip, codec_plan.h)
SUBCAP = 512                       # sub-sequences recorded per candidate block (one slot is kept for the end record)
SUB_BITS = 1024                    # bits per sub-sequence, at most
CHAIN_INLINE_BYTES = 4096          # longest unannounced Huffman block the chain walk counts itself
CHAIN_LDS_CAND = 1024              # candidates of a chunk the chain walk holds in LDS
SCAN_FINAL_ZONE = 256 * 1024       # bytes before the end of a stream in which the scan looks at BFINAL = 1 candidates
SCAN_MIN_BITS = 100                # a candidate has at least this many bits of stream behind its first bit
WAVE_ROUND_BITS = 1024 * 512       # bits the wave decoder takes from a block in one round
ROWCAP = 192                       # tokens pass A keeps per sub-sequence
SUB_MIN = 256                      # the shortest sub-sequence pass A cuts a block into when it takes the block for a short one


def cand_cap(c_len):
    return c_len // 4096 + 64


def true_cap(c_len):
    return 2 * cand_cap(c_len)


LIMITS = ('subcap_under', 'subcap_over', 'true_cap', 'cand_cap', 'chain_lds_cand', 'inline_at', 'inline_over', 'final_zone', 'wave_round',
          'rowcap', 'subcap_retry')


class Case:
    def __init__(self, stream, data, n, shape, limit=None, large=False, z_shape=None, writer=None):
        self.stream = stream
        self.data = data                    # None: refused
        self.n = n                          # the output size a caller states (len(data) for a valid stream)
        self.shape = shape                  # [(btype, tokens | stored length)] of a valid stream
        self.limit = limit
        self.large = large
        self.z_shape = stream if z_shape is None else z_shape       # what deflate_shape.blocks() is given
        self.block_bits = writer.block_bits if writer is not None else None
        self.block_out = writer.block_out if writer is not None else None


class _Catalogue(dict):
    def ok(self, name, w, limit=None, large=False, **zw):
        data = D.expand(w.tokens)
        z = D.zwrap(w, data, **zw)
        assert name not in self, name
        zs = D.zwrap(w, data, **{k: v for k, v in zw.items() if k != 'trailing'}) if 'trailing' in zw else None
        self[name] = Case(z, data, len(data), list(w.shape), limit, large, zs, w)

    def ok_bytes(self, name, z, data, shape):
        assert name not in self, name
        self[name] = Case(z, data, len(data), shape)

    def bad(self, name, z, n):
        assert name not in self, name
        self[name] = Case(bytes(z), None, n, None)


def rnd(n, seed, k=256, lo=0):
    return (np.random.RandomState(seed).randint(0, k, size=n) + lo).astype(np.uint8).tobytes()


FLAT8 = [8] * 255 + [0, 8]                         # literals 0 .. 254 and the end-of-block code: 256 codes of 8 bits
# 1, 2, .., 14, 15, 15: a complete code with one code of every length and the all-ones 15-bit code
STAIR_LIT = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 6: 7, 7: 8, 8: 9, 9: 10, 10: 11, 257: 12, 258: 13, 285: 14, 11: 15, 256: 15}
STAIR_DIST = list(range(1, 16)) + [15]             # distance codes 0 .. 15: code 7 has 8 bits, 8 has 9, 14 and 15 have 15


def lens_of(table, n):
    out = [0] * n
    for s, l in table.items():
        out[s] = l
    return out


# ---- valid streams ---------------------------------------------------------------------------------------------------------
def _emit(w, kind, tokens, final, **kw):
    (w.fixed if kind == 'fixed' else w.dynamic)(tokens, final, **kw)


def _lengths_and_distances(C):
    for kind in ('fixed', 'dynamic'):
        for spell in (284, 285):
            w = D.Writer()
            _emit(w, kind, list(b'abcdefgh') + [(258, 8, spell), 120, (258, 3, spell), (258, 1, spell)], True)
            C.ok('len258_as_%d_%s' % (spell, kind), w)
        toks = list(rnd(40, 1, 26, 97))
        for i in range(29):
            toks += [(D.LEN_BASE[i], 7), 65 + i]
            top = D.LEN_BASE[i] + (1 << D.LEN_EXTRA[i]) - 1
            toks += [(258, 11, 284), 66, (257, 5)] if i == 27 else [(top, 11)]
        w = D.Writer()
        _emit(w, kind, toks, True)
        C.ok('every_length_code_%s' % kind, w)
        toks = [rnd(32768, 2, 16)]
        for j in range(30):
            toks += [(3, D.DIST_BASE[j]), 200 + j, (4, D.DIST_BASE[j] + (1 << D.DIST_EXTRA[j]) - 1)]
        w = D.Writer()
        _emit(w, kind, toks, True)
        C.ok('every_distance_code_%s' % kind, w)


def _reach_byte_zero(C):
    for kind in ('fixed', 'dynamic'):
        for n in (1, 2, 8, 9):
            w = D.Writer()
            _emit(w, kind, list(rnd(n, 3 + n, 26, 97)) + [(5, n), 33, (3 + n, n + 6)], True)
            C.ok('reach0_nout%d_%s' % (n, kind), w)
    for kind in ('fixed', 'dynamic'):
        w = D.Writer()
        w.dynamic([rnd(32768, 4, 16)], False)
        _emit(w, kind, [(10, 32768), 7, (258, 32768), rnd(60, 5, 16)], True)
        C.ok('reach0_nout32768_%s_block' % kind, w)
    w = D.Writer()                                      # at the start of a dynamic block the scan announces
    w.dynamic([rnd(2000, 6, 64)], False)
    w.dynamic([(20, 2000), rnd(300, 7, 64), (30, 2320)], False)
    w.dynamic([(258, 2350), rnd(300, 8, 64)], True)
    C.ok('reach0_start_of_scanned_block', w)
    w = D.Writer()
    w.fixed(list(rnd(700, 9, 64)), False)
    w.fixed([(9, 700), 1, 2, 3], False)
    w.stored(rnd(500, 10), False)
    w.fixed([(258, 1212), (11, 500)], False)
    w.stored(rnd(77, 11), False)
    w.dynamic([(100, 1558), (3, 77), rnd(50, 12, 64)], True)
    C.ok('reach0_start_of_fixed_and_after_stored', w)


def _overlaps(C):
    for kind in ('fixed', 'dynamic'):
        toks = list(b'123456789')
        for d in range(1, 10):
            for ln in (3, 8, 9, 10, 11, 16, 17, 258):
                toks += [(ln, d), 97 + d]
        w = D.Writer()
        _emit(w, kind, toks, True)
        C.ok('overlapping_copies_%s' % kind, w)
    w = D.Writer()                                      # 33 pieces per token: a sub-sequence of ~340 such tokens overflows a row
    w.dynamic([rnd(100, 13, 64)], False)
    w.dynamic([90] + [(258, 1)] * 600, False)
    w.dynamic([rnd(100, 14, 64), (258, 300)], True)
    C.ok('run_of_258_at_distance_1', w, limit='rowcap')


def _code_lengths(C):
    lit_eob = lens_of(STAIR_LIT, 286)
    lit_len = lens_of({**STAIR_LIT, 256: 15, 11: 0, 270: 15}, 286)      # the all-ones code is length symbol 270 (23 .. 26)
    body = list(rnd(300, 15, 11)) + [8, 7, 10, 9, 8, 7]
    copies = []
    for j in range(16):
        d = D.DIST_BASE[j] + (1 << D.DIST_EXTRA[j]) - 1
        copies += [(3, d), (4, D.DIST_BASE[j]), (258, d), j % 11]
    w = D.Writer()
    w.dynamic(body + [11] + copies + [11, 11], False, lit_lens=lit_eob, dist_lens=STAIR_DIST)
    w.dynamic(body + copies, True, lit_lens=lit_eob, dist_lens=STAIR_DIST)
    C.ok('codes_of_8_9_15_bits_eob_all_ones', w)
    w = D.Writer()
    w.dynamic(body + copies + [(23, 255), 1, (26, 256)] + copies, False, lit_lens=lit_len, dist_lens=STAIR_DIST)
    w.dynamic(body[:40] + [(24, 17)], True, lit_lens=lit_len, dist_lens=STAIR_DIST)
    C.ok('codes_of_8_9_15_bits_length_all_ones', w)


def _incomplete_but_accepted(C):
    only_eob = [0] * 256 + [1]
    w = D.Writer()
    w.dynamic([], False, lit_lens=only_eob, dist_lens=[0])
    w.fixed(list(b'after an empty block'), False)
    w.dynamic([], False, lit_lens=only_eob, dist_lens=[0])
    w.dynamic([rnd(200, 16, 64), (30, 200)], False)
    w.dynamic([], True, lit_lens=only_eob, dist_lens=[0])
    C.ok('only_code_is_a_1_bit_end_of_block', w)
    w = D.Writer()
    w.dynamic(list(b'ab') + [(5, 1), 99, (258, 1), 100, (3, 1)], False, dist_lens=[1])
    w.dynamic(list(rnd(12, 17, 26, 97)) + [(5, 7), 99, (40, 8), 100, (3, 7)], True, dist_lens=[0, 0, 0, 0, 0, 1])
    C.ok('one_distance_code_used', w)
    w = D.Writer()
    w.dynamic([rnd(500, 18, 32)], False, dist_lens=[0])
    w.dynamic([rnd(50, 19, 32)], True, dist_lens=[0])
    C.ok('no_distance_code_literals_only', w)


def _header_counts(C):
    # HCLEN 4 names lengths for the symbols 16, 17, 18 and 0 only: no length but 0 can be stated, no end-of-block code, so no
    # valid block has it (it is among the refused cases).  The smallest HCLEN of a valid block is 5 (symbol 8 too).
    w = D.Writer()
    w.dynamic([rnd(400, 20, 255)], False, lit_lens=FLAT8, dist_lens=[0], hlit=257, hdist=1, hclen=5)
    w.dynamic([rnd(100, 21, 255)], True, lit_lens=FLAT8, dist_lens=[0], hlit=257, hdist=1, hclen=5)
    C.ok('hlit257_hdist1_hclen5', w)
    lit = lens_of(STAIR_LIT, 286)
    dist = [0] * 30
    for j, l in enumerate(STAIR_DIST[:-1]):
        dist[j] = l
    dist[29] = 15
    w = D.Writer()
    toks = list(rnd(300, 22, 11)) + [(258, 100), (3, 1), 11]
    w.dynamic([rnd(32768, 23, 11)], False)
    w.dynamic(toks + [(3, 32768), (258, 24577)], False, lit_lens=lit, dist_lens=dist, hlit=286, hdist=30, hclen=19)
    w.dynamic(toks, True, lit_lens=lit, dist_lens=dist, hlit=286, hdist=30, hclen=19)
    C.ok('hlit286_hdist30_hclen19', w)
    six = lens_of({0: 2, 1: 2, 256: 3, 257: 3, 258: 3, 259: 3}, 260)
    w = D.Writer()                                      # one 16 repeats symbol 256's length over 257 .. 259 and the first three distance lengths
    items = [2, 2, (18, 138), (18, 116), 3, (16, 6), (16, 5)]
    toks = [0, 1, 1, 0, (3, 1), (4, 2), (5, 3), 1, (3, 8), (4, 12), (5, 16), (3, 5), 0]
    w.dynamic(toks, False, lit_lens=six, dist_lens=[3] * 8, cl_items=items)
    w.dynamic(toks, True, lit_lens=six, dist_lens=[3] * 8, cl_items=items)
    C.ok('item_16_carries_a_length_into_the_distance_lengths', w)
    w = D.Writer()                                      # 10 zero lengths end the one alphabet, 4 begin the other: one 18 item
    items = [2, 2, (18, 138), (18, 116), 3, (16, 3), (18, 14), 1, 1]
    toks = [0, 1, 1, 0, 1, 1, 0, 1, 0, (3, 5), (4, 8), (5, 6), 1]
    w.dynamic(toks, False, lit_lens=six + [0] * 10, dist_lens=[0, 0, 0, 0, 1, 1], hlit=270, cl_items=items)
    w.dynamic(toks, True, lit_lens=six + [0] * 10, dist_lens=[0, 0, 0, 0, 1, 1], hlit=270, cl_items=items)
    C.ok('item_18_spans_both_alphabets', w)
    r = np.random.RandomState(24)
    lit = D.limited_lengths([int(x) for x in r.randint(1, 2000, size=286)], 15)
    dist = D.limited_lengths([int(x) for x in r.randint(1, 2000, size=30)], 15)
    w = D.Writer()
    toks = [rnd(400, 25)] + [(3 + k, 1 + 13 * k) for k in range(25)]
    w.dynamic(toks, False, lit_lens=lit, dist_lens=dist, hlit=286, hdist=30, cl_items=lit + dist)
    w.dynamic(toks, True, lit_lens=lit, dist_lens=dist, hlit=286, hdist=30, cl_items=lit + dist)
    C.ok('header_of_316_explicit_lengths', w)


def _empty_blocks(C):
    w = D.Writer()
    w.fixed(list(b'xyz'), False)
    for _ in range(300):
        w.stored(b'', False)
    w.fixed([(6, 3), 65], True)
    C.ok('300_empty_stored_blocks', w, limit='true_cap')
    w = D.Writer()
    w.stored(b'', False)
    w.dynamic([rnd(300, 26, 64)], False)
    w.stored(b'', False)
    w.stored(b'', False)
    w.fixed([(6, 3), 65], False)
    w.stored(b'', True)
    C.ok('empty_stored_blocks_between', w)
    w = D.Writer()
    for k in range(5):
        w.fixed([], False)
    w.dynamic([rnd(300, 27, 64)], False)
    w.fixed([], False)
    w.fixed([(6, 3), 65], False)
    w.fixed([], True)
    C.ok('empty_fixed_blocks', w)
    w = D.Writer()
    w.dynamic([], False)
    w.dynamic([rnd(300, 28, 64)], False)
    for k in range(3):
        w.dynamic([], False)
    w.dynamic([(6, 3), 65], False)
    w.dynamic([], True)
    C.ok('empty_dynamic_blocks', w)
    data = inputs.textlike(3000, 29)                   # zlib's own empty fixed blocks: what Z_PARTIAL_FLUSH writes
    co = zlib.compressobj(6)
    z = b''.join(co.compress(data[i:i + 500]) + co.flush(zlib.Z_PARTIAL_FLUSH) for i in range(0, len(data), 500)) + co.flush()
    C.ok_bytes('zlib_partial_flush', z, data, None)


def _stored(C):
    w = D.Writer()
    w.stored(rnd(65535, 30), False)
    w.stored(rnd(10, 31), False)
    w.fixed([(258, 32768), (10, 10)], True)
    C.ok('stored_len_65535', w)
    w = D.Writer()                                      # a fixed block of k 8-bit and j 9-bit literals ends at bit phase (2 + j) % 8
    for j in range(8):
        w.fixed([65] * (j + 1) + [200] * j, False)
        w.stored(rnd(20 + j, 32 + j), False)
    w.fixed([(30, 100)], True)
    C.ok('stored_at_every_bit_phase', w)
    for name, x in (('text', inputs.textlike(330000, 40)), ('ar1', inputs.ar1_stream(2200, 64))):
        inner = zlib.compress(x, 6)
        w = D.Writer()
        for i in range(0, len(inner), 40000):
            w.stored(inner[i:i + 40000], i + 40000 >= len(inner))
        C.ok('deflate_stream_in_stored_blocks_%s' % name, w)
        w = D.Writer()
        w.fixed([inner], True)
        C.ok('deflate_stream_as_fixed_literals_%s' % name, w)


def _chain_inline(C):
    for total, limit in ((4096, 'inline_at'), (4097, 'inline_over')):
        w = D.Writer()
        w.dynamic([rnd(3000, 41, 64)], False)
        toks = [rnd(1000, 42, 64), (258, 3000), (258, 1)] + [(200, 777)] * 12
        toks.append(rnd(total - len(D.expand(w.tokens + toks)) + 3000, 43, 64))
        w.fixed(toks, False)
        w.dynamic([rnd(200, 44, 64), (50, 4000)], True)
        C.ok('fixed_block_of_%d_bytes_after_a_dynamic_block' % total, w, limit=limit)


def _long_blocks(C):
    per = SUB_BITS // 8
    for name, ntok, limit in (('just_under_511_subsequences', 511 * per - 1, 'subcap_under'), ('just_over_511_subsequences', 511 * per, 'subcap_over'),
                              ('of_three_times_511_subsequences', 3 * 511 * per + 77, 'subcap_over')):
        w = D.Writer()
        w.dynamic([rnd(200, 45, 64)], False)
        w.dynamic([rnd(ntok, 46, 255)], False, lit_lens=FLAT8, dist_lens=[0])
        w.dynamic([(258, 32768), rnd(200, 47, 64), (100, 30000)], True)
        C.ok('dynamic_block_' + name, w, limit=limit, large=name.startswith('of_three'))
    w = D.Writer()                                      # no candidate: the wave decoder takes it, in more than one round
    w.fixed([rnd(66000, 48, 144)], False)
    w.dynamic([(258, 32768), rnd(200, 49, 64)], True)
    C.ok('fixed_block_of_two_wave_rounds', w, limit='wave_round')


def rev8(b):
    return int('{:08b}'.format(b)[::-1], 2)


ALL_LITERALS = [8] * 255 + [9, 9]                  # literal v < 255 has the 8-bit code v: its bits in the stream are the byte rev8(v)


def _false_headers_in_a_block(C):
    # A dynamic block whose BITS hold a deflate stream: the scan announces the inner stream's block headers as candidates, the
    # first of them 16 bits into the body.  Pass A takes the next candidate for the block's end, cuts the block into
    # sub-sequences of the shortest kind (256 bits), runs out of records after 511 of them and starts again at full length.
    for seed in range(64):                             # (a byte 255 is a 9-bit literal and shifts what follows: none in the first header)
        x = inputs.ar1_stream(800, 64, seed)
        co = zlib.compressobj(6)
        inner = b''.join(co.compress(x[i:i + 3000]) + co.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(x), 3000)) + co.flush()
        if 255 not in inner[:200]:
            break
    w = D.Writer()
    w.dynamic([rnd(200, 64, 64)], False)
    w.dynamic([bytes(rev8(b) for b in inner)], False, lit_lens=ALL_LITERALS, dist_lens=[0])
    w.dynamic([(258, 30000), rnd(200, 65, 64), (100, 200)], True)
    C.ok('dynamic_block_with_block_headers_in_its_bits', w, limit='subcap_retry')


def _many_blocks(C):
    r = np.random.RandomState(50)
    w = D.Writer()
    for k in range(100):
        w.dynamic([int(x) for x in r.randint(97, 123, size=1 + k % 2)], False)
    w.dynamic([(40, 100), rnd(60, 51, 64)], True)
    C.ok('100_tiny_dynamic_blocks', w, limit='cand_cap')
    w = D.Writer()                                      # zero bytes hold no block type 2: the filler adds no candidate
    for k in range(1100):
        w.dynamic([int(x) for x in r.randint(97, 123, size=1 + k % 2)], False)
        w.stored(bytes(4000), False)
    w.dynamic([(40, 12000), rnd(60, 52, 64)], True)
    C.ok('1100_tiny_dynamic_blocks_in_stored_filler', w, limit='chain_lds_cand', large=True)


def _far_final_block(C):
    w = D.Writer()
    w.dynamic([rnd(500, 53, 64)], False)
    w.dynamic([rnd(300000, 54, 255)], True, lit_lens=FLAT8, dist_lens=[0])
    C.ok('final_block_starts_before_the_final_zone', w, limit='final_zone', large=True)


def _alternating(C):
    r = np.random.RandomState(55)
    w = D.Writer()
    w.fixed(list(rnd(300, 56, 64)), False)
    seen = {0: set(), 1: set(), 2: set()}
    k = 0
    while any(len(s) < 8 for s in seen.values()):
        kind = int(r.randint(0, 3))                   # (in a fixed order the block behind a stored one would always start a byte)
        nout = len(D.expand(w.tokens))
        seen[kind].add(w.bitpos % 8)
        if kind == 0:
            w.stored(rnd(int(r.randint(1, 60)), 57 + k), False)
        else:
            toks = [(int(r.randint(3, 259)), min(32768, nout - int(r.randint(0, min(nout, 200)))))]          # reaches into the blocks before
            toks += [int(x) for x in r.randint(0, 256, size=int(r.randint(0, 12)))]
            toks += [(int(r.randint(3, 40)), int(r.randint(1, 30)))]
            _emit(w, 'fixed' if kind == 1 else 'dynamic', toks, False, **({'maxbits': int(r.randint(7, 16))} if kind == 2 else {}))
        k += 1
        assert k < 600
    w.fixed([(258, min(32768, len(D.expand(w.tokens))))], True)
    C.ok('block_types_alternate_at_every_bit_phase', w)


def _zlib_header(C):
    toks = list(b'header ') + [(20, 7), (3, 1)]
    for cinfo in range(8):
        w = D.Writer()
        w.fixed(toks, True)
        C.ok('cinfo_%d' % cinfo, w, cmf=(cinfo << 4) | 8)
    for flevel in range(4):
        w = D.Writer()
        w.dynamic(toks, True)
        C.ok('flevel_%d' % flevel, w, flg=D.flg_for(0x78, flevel))
    w = D.Writer()
    w.dynamic(toks, True)
    C.ok('trailing_bytes_after_the_check_value', w, trailing=b'\x78\x9c trailing bytes \x05\x00')


def _resolver_segments(C):
    # the resolver cuts a chunk by groups of 64 tokens into segments that each produce a window (32768 + 512 bytes) or more:
    # 140 000 one-byte tokens are cut into 2 or 4.  The copy lies 50 tokens behind the cuts at 1/4, 1/2 and 3/4 and reaches
    # 51 bytes before them -- legal there, and one byte too far at byte 100 of the first segment (the refused twin below).
    n = 140000
    lits = rnd(n, 58, 4)
    cuts = sorted({((n + 63) // 64 + s - 1) // s * 64 * j for s in (2, 4) for j in range(1, s)})
    toks, at = [], 0
    for c in cuts:
        toks += [lits[at:c + 50], (3, 101)]
        at = c + 50
    toks.append(lits[at:])
    w = D.Writer()
    w.dynamic(toks, True)
    C.ok('distance_101_behind_the_start_of_a_later_segment', w)
    w = D.Writer()
    w.dynamic([lits[:100], (3, 101), lits[100:]], True)
    C.bad('distance_101_at_byte_100_of_the_first_segment', D.zwrap(w, b''), n + 3)


# ---- refused streams -----------------------------------------------------------------------------------------------------
def _forbidden_symbols(C):
    for s in (286, 287):
        w = D.Writer()
        w.fixed(list(b'abc') + [('raw', 'l', s, 0, 0)] + list(b'def'), True)
        C.bad('literal_length_symbol_%d_fixed' % s, D.zwrap(w, b'abcdef'), 6)
    for s in (30, 31):
        w = D.Writer()
        w.fixed(list(b'abcdefgh') + [('raw', 'l', 257, 0, 0), ('raw', 'd', s, 0, 0)] + list(b'def'), True)
        C.bad('distance_symbol_%d_fixed' % s, D.zwrap(w, b'abcdefghabcdef'), 14)
    # The same symbols as a decoder reads them that continues the tables past their ends -- length 323 and 387 with 6 extra bits,
    # distance 32769 with 14 extra bits, which wraps to distance 1 in a 15-bit field -- and with the check value of the bytes
    # such a decoder produces: nothing but the symbol itself refuses these streams.
    for s, base in ((286, 323), (287, 387)):
        w = D.Writer()
        w.fixed(list(b'abcdefgh') + [('raw', 'l', s, 0, 6), ('raw', 'd', 0, 0, 0)] + list(b'def'), True)
        C.bad('literal_length_symbol_%d_with_the_check_value_of_length_%d' % (s, base), D.zwrap(w, b'abcdefgh' + b'h' * base + b'def'), 11 + base)
    w = D.Writer()
    w.fixed(list(b'abcdefgh') + [('raw', 'l', 257, 0, 0), ('raw', 'd', 30, 0, 14)] + list(b'def'), True)
    C.bad('distance_symbol_30_with_the_check_value_of_distance_1', D.zwrap(w, b'abcdefghhhhdef'), 14)
    lit = D.limited_lengths([1] * 286, 15)
    for nlen in (287, 288):
        w = D.Writer()
        w.dynamic(list(b'abc'), True, lit_lens=lit + [0] * (nlen - 286), dist_lens=[1, 1], hlit=nlen)
        C.bad('hlit_%d' % nlen, D.zwrap(w, b'abc'), 3)
    for ndist in (31, 32):
        w = D.Writer()
        w.dynamic(list(b'abc'), True, lit_lens=lit, dist_lens=[1, 1] + [0] * (ndist - 2), hdist=ndist)
        C.bad('hdist_%d' % ndist, D.zwrap(w, b'abc'), 3)


def _too_far_back(C):
    for kind in ('fixed', 'dynamic'):
        w = D.Writer()
        _emit(w, kind, [97, (3, 2), 98, 99], True)
        C.bad('distance_2_at_byte_1_%s' % kind, D.zwrap(w, b''), 6)
        w = D.Writer()
        w.fixed(list(b'0123456789'), False)
        _emit(w, kind, [(3, 11), 98, 99], True)
        C.bad('distance_11_at_byte_10_start_of_%s_block' % kind, D.zwrap(w, b''), 15)
    w = D.Writer()
    w.dynamic([rnd(32767, 59, 16), (3, 32768), 1, 2], True)
    C.bad('distance_32768_at_byte_32767', D.zwrap(w, b''), 32772)
    w = D.Writer()
    w.dynamic([rnd(2000, 60, 64)], False)
    w.dynamic([(20, 2001), rnd(300, 61, 64)], False)
    w.dynamic([rnd(300, 62, 64)], True)
    C.bad('distance_2001_at_byte_2000_start_of_scanned_block', D.zwrap(w, b''), 2620)


def _bad_trees(C):
    two = lens_of({97: 1, 98: 1}, 257)
    w = D.Writer()
    w.dynamic([97, 98, 97], True, lit_lens=two, dist_lens=[0], eob=False)
    C.bad('no_end_of_block_code', D.zwrap(w, b'aba'), 3)
    w = D.Writer()
    w.dynamic([], True, lit_lens=[0] * 257, dist_lens=[0], hclen=4, cl_lens=lens_of({0: 1, 18: 1}, 19), eob=False)
    C.bad('hclen_4', D.zwrap(w, b''), 1)
    good = lens_of({97: 2, 98: 2, 99: 2, 256: 2}, 257)
    cl = {0: 2, 2: 2, 18: 2, 1: 2}                       # what the header of `good` needs: a complete code-length code
    w = D.Writer()
    w.dynamic([97, 98], True, lit_lens=good, dist_lens=[1, 1], cl_lens=lens_of({**cl, 1: 1}, 19))
    C.bad('code_length_code_over_subscribed', D.zwrap(w, b'ab'), 2)
    w = D.Writer()
    w.dynamic([97, 98], True, lit_lens=good, dist_lens=[1, 1], cl_lens=lens_of({**cl, 1: 3}, 19))
    C.bad('code_length_code_incomplete', D.zwrap(w, b'ab'), 2)
    w = D.Writer()
    w.dynamic([97, 98], True, lit_lens=lens_of({97: 1, 98: 1, 256: 1}, 257), dist_lens=[1, 1])
    C.bad('literal_length_code_over_subscribed', D.zwrap(w, b'ab'), 2)
    w = D.Writer()
    w.dynamic([97, 98], True, lit_lens=lens_of({97: 2, 98: 2, 256: 2}, 257), dist_lens=[1, 1])
    C.bad('literal_length_code_incomplete', D.zwrap(w, b'ab'), 2)
    w = D.Writer()
    w.dynamic([97, 98], True, lit_lens=good, dist_lens=[1, 1, 1])
    C.bad('distance_code_over_subscribed', D.zwrap(w, b'ab'), 2)
    w = D.Writer()
    w.dynamic([97, 98], True, lit_lens=good, dist_lens=[2, 2, 2])
    C.bad('distance_code_incomplete', D.zwrap(w, b'ab'), 2)
    w = D.Writer()
    w.dynamic([0], True, lit_lens=lens_of({0: 2, 1: 2, 2: 2, 256: 2}, 257), dist_lens=[1, 1],
              cl_items=[(16, 3), (18, 138), (18, 115), 2, 1, 1])
    C.bad('item_16_comes_first', D.zwrap(w, b''), 1)
    w = D.Writer()
    w.dynamic([97, 98], True, lit_lens=good, dist_lens=[1, 1], cl_items=[(18, 97), 2, 2, 2, (18, 138), (18, 18), 2, 1, (18, 11)])
    C.bad('repeat_runs_past_the_last_length', D.zwrap(w, b'ab'), 2)
    w = D.Writer()                                      # the distance tree's one code is '0': the bit behind symbol 257 is a 1
    w.dynamic([97, 98, 99, ('raw', 'l', 257, 1, 1), 97], True, dist_lens=[1])
    C.bad('unused_code_of_a_one_code_distance_tree', D.zwrap(w, b''), 7)
    w = D.Writer()
    w.dynamic([97, 98, 99, ('raw', 'l', 257, 0, 0), 97], True, dist_lens=[0])
    C.bad('length_symbol_without_a_distance_code', D.zwrap(w, b''), 7)


def _bad_blocks(C):
    w = D.Writer()
    w.fixed(list(b'abc'), False)
    w.bits(1, 1)
    w.bits(3, 2)
    w.bits(0, 29)
    C.bad('block_type_3', D.zwrap(w, b'abc'), 3)
    w = D.Writer()
    w.stored(b'0123456789', True, nlen=10 ^ 0xfffe)
    C.bad('stored_nlen_does_not_match', D.zwrap(w, b'0123456789'), 10)
    w = D.Writer()
    w.stored(b'0123456789', True, length=2000)
    C.bad('stored_len_past_the_end', D.zwrap(w, b'0123456789'), 2000)
    w = D.Writer()
    w.dynamic([rnd(3000, 63, 200), (100, 1000)], True)
    z = D.zwrap(w)
    hdr_end = w.block_bits[0][1] // 8 + 2
    C.bad('cut_in_the_dynamic_header', z[:hdr_end // 2], 3100)
    C.bad('cut_in_the_block', z[:hdr_end + 1000], 3100)
    C.bad('cut_before_the_check_value', z[:-4], 3100)
    C.bad('cut_in_the_check_value', z[:-1], 3100)
    C.bad('wrong_check_value', z[:-4] + ((int.from_bytes(z[-4:], 'big') + 1) & 0xffffffff).to_bytes(4, 'big'), 3100)
    body = z[2:]
    C.bad('header_fcheck_wrong', bytes([0x78, 0x9d]) + body, 3100)
    C.bad('header_cm_7', bytes([0x77, D.flg_for(0x77)]) + body, 3100)
    C.bad('header_cinfo_8', bytes([0x88, D.flg_for(0x88)]) + body, 3100)
    C.bad('header_fdict', bytes([0x78, D.flg_for(0x78, 2, 1)]) + body, 3100)


@functools.lru_cache(maxsize=None)
def catalogue():
    """name -> Case, built once per process."""
    C = _Catalogue()
    for part in (_lengths_and_distances, _reach_byte_zero, _overlaps, _code_lengths, _incomplete_but_accepted, _header_counts, _empty_blocks,
                 _stored, _chain_inline, _long_blocks, _false_headers_in_a_block, _many_blocks, _far_final_block, _alternating, _zlib_header, _resolver_segments,
                 _forbidden_symbols, _too_far_back, _bad_trees, _bad_blocks):
        part(C)
    return C


def cases():
    """name -> (stream, data or None); None: zlib refuses the stream."""
    return {name: (c.stream, c.data) for name, c in catalogue().items()}


# the valid streams that are also given with a wrong size and with a wrong check value
SIZE_CASES = ('len258_as_284_dynamic', 'overlapping_copies_fixed', 'stored_at_every_bit_phase', '300_empty_stored_blocks',
              'codes_of_8_9_15_bits_eob_all_ones', 'dynamic_block_just_over_511_subsequences')


def wrong_check(z):
    return z[:-4] + bytes([z[-4] ^ 0x10]) + z[-3:]
