"""A reader of zlib streams (RFC 1950 / 1951), pure Python: which blocks a stream has and what their headers hold.

It walks the blocks of a zlib stream -- stdlib ``zlib.compress``'s, a hand-built one, or the device's bytes once they have been
copied to the host (any bytes-like object) -- and decodes no match beyond its length.  Its purpose is to state which edges of
the block encoder and of the header decoder a test case reaches (tests/block_cases.py, tests/test_block_cases.py), to name the
block a differing byte lies in (tests/test_gpu_block_edges.py), and to say where the block that completes a wanted prefix of the
output ends (tests/prefix_cases.py).

``blocks(z)`` returns one dict per block:

    btype, last     0 stored / 1 fixed / 2 dynamic, BFINAL
    bit_start       bit offset of the block's first (BFINAL) bit in the stream, the two zlib header bytes included
    bit_end         bit offset behind the block (behind the end-of-block code; a stored block's last byte)
    nout            bytes the block produces: 1 per literal, the copy length per match, LEN for a stored block
    stored:         pad (padding bits between the 3 block-type bits and LEN), len (LEN)
    dynamic:        hlit, hdist, hclen (the COUNTS: 257 .. 286, 1 .. 30, 4 .. 19),
                    bl_lens (the 19 bit-length code lengths, by symbol), bl_max,
                    l_max_len, d_max_len (longest literal/length and distance code length),
                    items (the (16 | 17 | 18, repeat) items of the header, in order),
                    hdr_bits (HLIT .. the last code-length code: the header WITHOUT the 3 block-type bits, which is what
                    the oracle reports and what the encoder's header image holds)
    fixed, dynamic: ntok (tokens, the end-of-block code not counted), body_bits (the tokens' bits and the end-of-block code's)
"""

BL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)


class _Bits:
    def __init__(self, data, pos):
        self.d = data + bytes(4)                       # (zeros behind the end: peek() may look past the last code)
        self.n = 8 * len(data)
        self.pos = pos

    def peek(self, k):                                 # k <= 16
        p = self.pos
        return (int.from_bytes(self.d[p >> 3:(p >> 3) + 4], 'little') >> (p & 7)) & ((1 << k) - 1)

    def take(self, k):
        if self.pos + k > self.n:
            raise ValueError('stream ends inside a block')
        x = self.peek(k)
        self.pos += k
        return x


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = r << 1 | (code & 1)
        code >>= 1
    return r


def _decoder(lens):
    """Canonical Huffman code of `lens` -> (max length, table indexed by the next `max length` stream bits -> (symbol, length))."""
    mx = max(lens)
    if mx == 0:
        return 0, []
    count = [0] * (mx + 1)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = [None] * (1 << mx)
    for sym, l in enumerate(lens):
        if l:
            r = _rev(nxt[l], l)
            nxt[l] += 1
            for hi in range(0, 1 << mx, 1 << l):
                table[hi | r] = (sym, l)
    return mx, table


def _sym(bits, dec):
    mx, table = dec
    e = table[bits.peek(mx)] if mx else None
    if e is None:
        raise ValueError('no such code')
    bits.take(e[1])
    return e[0]


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _decoder([5] * 30))
    return _FIXED


def _body(bits, ldec, ddec):
    """(tokens, bytes produced) of a block body; the end-of-block code is consumed.  One 8-byte window per token holds all of it
    (15 + 5 + 15 + 13 bits at most), so the loop does without _Bits' calls: the catalogues walk megabytes of streams."""
    (lmx, ltab), (dmx, dtab) = ldec, ddec
    if not lmx:
        raise ValueError('no such code')
    d, pos, n, frm = bits.d, bits.pos, bits.n, int.from_bytes
    lmask, dmask = (1 << lmx) - 1, (1 << dmx) - 1
    ntok = nout = 0
    while True:
        w = frm(d[pos >> 3:(pos >> 3) + 8], 'little') >> (pos & 7)
        e = ltab[w & lmask]
        if e is None:
            raise ValueError('no such code')
        s, used = e
        if s > 256:
            x = LEN_EXTRA[s - 257]
            nout += LEN_BASE[s - 257] + ((w >> used) & ((1 << x) - 1))
            used += x
            e = dtab[(w >> used) & dmask] if dmx else None
            if e is None:
                raise ValueError('no such code')
            bits.pos = pos + used + e[1]
            bits.take(DIST_EXTRA[e[0]])                        # (through take(): tests count the 13-bit ones)
            pos, used = bits.pos, 0
        pos += used
        if pos > n:
            raise ValueError('stream ends inside a block')
        if s == 256:
            bits.pos = pos
            return ntok, nout
        ntok += 1
        if s < 256:
            nout += 1


def blocks(z):
    """The blocks of the zlib stream `z` (see the module's docstring)."""
    z = bytes(z)
    if len(z) < 6 or (z[0] & 15) != 8 or ((z[0] << 8) | z[1]) % 31 or z[1] & 0x20:
        raise ValueError('not a zlib stream without a preset dictionary')
    bits = _Bits(z[:-4], 16)
    out = []
    while True:
        b = {'bit_start': bits.pos}
        b['last'] = bits.take(1)
        b['btype'] = bits.take(2)
        if b['btype'] == 0:
            b['pad'] = -bits.pos % 8
            bits.take(b['pad'])
            b['len'] = bits.take(16)
            if bits.take(16) != b['len'] ^ 0xffff:
                raise ValueError('stored block: LEN / NLEN')
            if bits.pos + 8 * b['len'] > bits.n:
                raise ValueError('stream ends inside a block')
            bits.pos += 8 * b['len']
            b['nout'] = b['len']
        elif b['btype'] == 1:
            t0 = bits.pos
            b['ntok'], b['nout'] = _body(bits, *_fixed())
            b['body_bits'] = bits.pos - t0
        elif b['btype'] == 2:
            h0 = bits.pos
            b['hlit'], b['hdist'], b['hclen'] = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
            bl = [0] * 19
            for k in range(b['hclen']):
                bl[BL_ORDER[k]] = bits.take(3)
            b['bl_lens'], b['bl_max'] = bl, max(bl)
            dec = _decoder(bl)
            lens, items = [], []
            while len(lens) < b['hlit'] + b['hdist']:
                s = _sym(bits, dec)
                if s < 16:
                    lens.append(s)
                    continue
                rep = bits.take((2, 3, 7)[s - 16]) + (3, 3, 11)[s - 16]
                if s == 16 and not lens:
                    raise ValueError('code 16 with nothing before it')
                lens += [lens[-1] if s == 16 else 0] * rep
                items.append((s, rep))
            if len(lens) != b['hlit'] + b['hdist']:
                raise ValueError('a repeat runs past the last code length')
            b['items'] = items
            b['hdr_bits'] = bits.pos - h0
            ll, dl = lens[:b['hlit']], lens[b['hlit']:]
            b['l_max_len'], b['d_max_len'] = max(ll), max(dl)
            t0 = bits.pos
            b['ntok'], b['nout'] = _body(bits, _decoder(ll), _decoder(dl))
            b['body_bits'] = bits.pos - t0
        else:
            raise ValueError('reserved block type')
        b['bit_end'] = bits.pos
        out.append(b)
        if b['last']:
            if (bits.pos + 7) // 8 != len(z) - 4:
                raise ValueError('bytes between the last block and the check value')
            return out


def block_at(blks, byte):
    """Index of the block that byte offset `byte` of the stream lies in (the first one that reaches into that byte), or None
    for the two header bytes and the check value."""
    for i, b in enumerate(blks):
        if b['bit_start'] // 8 <= byte and 8 * byte < b['bit_end']:
            return i
    return None
