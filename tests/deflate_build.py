"""A writer of zlib streams (RFC 1950 / 1951) in plain Python: every block, tree, header count and run item as the caller
dictates, so that a test can state streams that no encoder writes -- and streams that no decoder may accept.

No zlib is used for the bit stream (zlib supplies adler32 only).  tests/inflate_cases.py builds its catalogue with it;
tests/test_inflate_cases.py certifies the catalogue against zlib.decompress and the oracle.

A TOKEN is
    an int 0..255                       a literal byte
    bytes                               literal bytes (what a stored block holds; in a Huffman block: one literal each)
    (length, distance)                  a copy, length 3..258, distance 1..32768; length 258 goes through code 285
    (258, distance, 284)                the same copy through length code 284 with extra bits 31 (285 may be given too)
    ('raw', 'l' | 'd', symbol, extra, extra_bits)
                                        one symbol of the literal/length ('l') or of the distance ('d') alphabet with
                                        `extra_bits` bits of value `extra` behind it, nothing checked (forbidden symbols;
                                        a length symbol without its distance)

    w = Writer(); w.dynamic(tokens, final=False); w.stored(b'...', final=True); z = zwrap(w)
    expand(w.tokens) == zlib.decompress(z)
"""
import heapq
import zlib

BL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32

_LEN_SYM = [0] * 259                       # length -> code index (0 .. 28); 258 -> 28 (code 285)
for _i in range(28):
    for _l in range(LEN_BASE[_i], LEN_BASE[_i] + (1 << LEN_EXTRA[_i])):
        if _l <= 258:
            _LEN_SYM[_l] = _i
_LEN_SYM[258] = 28


def dist_sym(d):
    """Distance code 0 .. 29 of distance d (1 .. 32768)."""
    lo, hi = 0, 29
    while lo < hi:
        m = (lo + hi + 1) // 2
        if DIST_BASE[m] <= d:
            lo = m
        else:
            hi = m - 1
    return lo


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = r << 1 | (code & 1)
        code >>= 1
    return r


def canonical(lens):
    """The canonical Huffman codes (RFC 1951, 3.2.2) of the code lengths `lens`: a list of codes, first bit most significant,
    0 where the length is 0.  Nothing is checked: an over-subscribed set of lengths gives codes that overflow their lengths."""
    mx = max(lens) if lens else 0
    count = [0] * (mx + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(0)
    return out


def kraft(lens, maxbits=15):
    """Sum of 2^(maxbits - l) over the non-zero lengths: 2^maxbits for a complete code."""
    return sum(1 << (maxbits - l) for l in lens if l)


def limited_lengths(freqs, maxbits):
    """Code lengths <= maxbits of a COMPLETE prefix code over the symbols with freqs > 0 (0 for the others).  Huffman's
    lengths, then the counts per length are repaired until the Kraft sum is 1 and handed out again by frequency.  With fewer
    than two used symbols the first unused symbols get a code too (a complete code has at least two)."""
    n = len(freqs)
    used = [i for i in range(n) if freqs[i] > 0]
    for i in range(n):
        if len(used) >= 2:
            break
        if i not in used:
            used.append(i)
    if len(used) < 2 or len(used) > (1 << maxbits):
        raise ValueError('no complete code of at most %d bits over %d symbols' % (maxbits, len(used)))
    heap = [(max(freqs[i], 0), k, (i,)) for k, i in enumerate(used)]
    heapq.heapify(heap)
    depth = dict.fromkeys(used, 0)
    k = len(heap)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for i in a + b:
            depth[i] += 1
        heapq.heappush(heap, (fa + fb, k, a + b))
        k += 1
    count = [0] * (maxbits + 1)
    for i in used:
        count[min(depth[i], maxbits)] += 1
    total = sum(count[l] << (maxbits - l) for l in range(1, maxbits + 1))
    while total > 1 << maxbits:                           # over-subscribed by the clamp: one leaf of the longest length goes
        count[maxbits] -= 1                                # beside a leaf moved one level down
        for l in range(maxbits - 1, 0, -1):
            if count[l]:
                count[l] -= 1
                count[l + 1] += 2
                break
        total -= 1
    order = sorted(used, key=lambda i: (-freqs[i], i))    # most frequent first: shortest codes
    lens = [0] * n
    at = 0
    for l in range(1, maxbits + 1):
        for i in order[at:at + count[l]]:
            lens[i] = l
        at += count[l]
    assert kraft(lens, maxbits) == 1 << maxbits
    return lens


def token_counts(tokens):
    """(literal/length counts [286], distance counts [30]) of a token list, the end-of-block symbol counted once."""
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        elif isinstance(t, (bytes, bytearray)):
            for b in t:
                lf[b] += 1
        elif t[0] == 'raw':
            f = lf if t[1] == 'l' else df
            if t[2] < len(f):
                f[t[2]] += 1
        else:
            lf[257 + (27 if len(t) > 2 and t[2] == 284 else _LEN_SYM[t[0]])] += 1
            df[dist_sym(t[1])] += 1
    return lf, df


def run_items(lens):
    """A code-length sequence as header items: an int 0..15 (a length) or (16 | 17 | 18, repeat), greedy, longest run first."""
    items, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        j = i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                items.append((18, r))
                run -= r
            if run >= 3:
                items.append((17, run))
                run = 0
            items += [0] * run
        else:
            items.append(v)
            run -= 1
            while run >= 3:
                r = min(run, 6)
                items.append((16, r))
                run -= r
            items += [v] * run
        i = j
    return items


class Writer:
    """Bits LSB-first into a bytearray through a small accumulator; Huffman codes MSB-first.  `tokens` collects what the blocks
    written so far produce (for expand()), `shape` one (btype, tokens or stored length) per block."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.tokens = []
        self.shape = []
        self.block_bits = []                              # (bit of the block's BFINAL, bit behind its header, bit behind the block)
        self.block_out = []                               # bytes each block produces

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bits(self, value, k):
        self.acc |= (value & ((1 << k) - 1)) << self.n
        self.n += k
        if self.n >= 64:
            self._flush()

    def _flush(self):
        nb = self.n >> 3
        self.out += (self.acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, 'little')
        self.acc >>= 8 * nb
        self.n -= 8 * nb

    def code(self, code, length):
        self.bits(_rev(code, length), length)

    def align(self):
        self.bits(0, -self.n % 8)
        self._flush()

    def raw_bytes(self, payload):
        assert self.n % 8 == 0
        self._flush()
        self.out += payload

    def getvalue(self):
        """The bytes so far, the last one padded with zero bits (the writer may go on)."""
        self._flush()
        return bytes(self.out) + (bytes([self.acc & 0xff]) if self.n else b'')

    # ---- blocks -------------------------------------------------------------------------------------------------------
    def stored(self, payload, final, length=None, nlen=None):
        """A stored block.  `length` / `nlen` override the LEN / NLEN fields (the payload is written as it is)."""
        p0 = self.bitpos
        self.bits(1 if final else 0, 1)
        self.bits(0, 2)
        self.align()
        ln = len(payload) if length is None else length
        self.bits(ln, 16)
        self.bits(ln ^ 0xffff if nlen is None else nlen, 16)
        self._flush()
        self.raw_bytes(payload)
        if payload:
            self.tokens.append(bytes(payload))
        self.shape.append((0, len(payload)))
        self.block_out.append(len(payload))
        self.block_bits.append((p0, p0 + 3, self.bitpos))

    def _body(self, tokens, lcode, dcode, eob=True):
        """The tokens and the end-of-block code, through tables of (reversed code, length) per symbol."""
        acc, n, out = self.acc, self.n, self.out
        ntok = 0

        def sym(tab, s, what):
            c = tab[s] if s < len(tab) else None
            if c is None or not c[1]:
                raise ValueError('%s symbol %d has no code' % (what, s))
            return c

        for t in tokens:
            if isinstance(t, int):
                c, l = lcode[t]
                if not l:
                    raise ValueError('literal %d has no code' % t)
                acc |= c << n
                n += l
                ntok += 1
            elif isinstance(t, (bytes, bytearray)):
                for b in t:
                    c, l = lcode[b]
                    if not l:
                        raise ValueError('literal %d has no code' % b)
                    acc |= c << n
                    n += l
                    if n >= 64:
                        out += (acc & 0xffffffffffffffff).to_bytes(8, 'little')
                        acc >>= 64
                        n -= 64
                ntok += len(t)
            elif t[0] == 'raw':
                c, l = sym(lcode if t[1] == 'l' else dcode, t[2], 'raw')
                acc |= c << n
                n += l
                acc |= (t[3] & ((1 << t[4]) - 1)) << n
                n += t[4]
                ntok += t[1] == 'l'
            else:
                ln, d = t[0], t[1]
                if not (3 <= ln <= 258 and 1 <= d <= 32768):
                    raise ValueError('copy (%d, %d)' % (ln, d))
                li = _LEN_SYM[ln]
                if len(t) > 2:
                    if ln != 258 or t[2] not in (284, 285):
                        raise ValueError('only length 258 has two spellings')
                    li = t[2] - 257
                c, l = sym(lcode, 257 + li, 'length')
                acc |= c << n
                n += l
                acc |= (ln - LEN_BASE[li]) << n
                n += LEN_EXTRA[li]
                di = dist_sym(d)
                c, l = sym(dcode, di, 'distance')
                acc |= c << n
                n += l
                acc |= (d - DIST_BASE[di]) << n
                n += DIST_EXTRA[di]
                ntok += 1
            if n >= 64:
                nb = n >> 3
                out += (acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, 'little')
                acc >>= 8 * nb
                n -= 8 * nb
        if eob:
            c, l = sym(lcode, 256, 'end-of-block')
            acc |= c << n
            n += l
        self.acc, self.n = acc, n
        self._flush()
        return ntok

    @staticmethod
    def _tables(lens):
        return [(_rev(c, l), l) for c, l in zip(canonical(lens), lens)]

    def _produce(self, tokens):
        made = [t for t in tokens if not (isinstance(t, tuple) and t[0] == 'raw')]
        self.tokens += made
        self.block_out.append(sum(1 if isinstance(t, int) else len(t) if isinstance(t, (bytes, bytearray)) else t[0] for t in made))

    def fixed(self, tokens, final, eob=True):
        p0 = self.bitpos
        self.bits(1 if final else 0, 1)
        self.bits(1, 2)
        ntok = self._body(tokens, self._tables(FIXED_LIT_LENS), self._tables(FIXED_DIST_LENS), eob)
        self._produce(tokens)
        self.shape.append((1, ntok))
        self.block_bits.append((p0, p0 + 3, self.bitpos))

    def dynamic(self, tokens, final, lit_lens=None, dist_lens=None, hlit=None, hdist=None, hclen=None, cl_items=None, cl_lens=None,
                maxbits=15, eob=True):
        """A dynamic block.  lit_lens / dist_lens: the code lengths by symbol (default: limited_lengths of the tokens' counts, at most
        `maxbits`); hlit / hdist / hclen: the COUNTS the header states (default: the smallest that hold the lengths; 257 .. 288,
        1 .. 32, 4 .. 19 can be written); cl_items: the code-length sequence as run_items() gives it (default: run_items of the
        hlit + hdist lengths); cl_lens: the 19 lengths of the code-length code by symbol (default: limited_lengths(.., 7))."""
        lf, df = token_counts(tokens)
        if lit_lens is None:
            lit_lens = limited_lengths(lf, maxbits)
        if dist_lens is None:
            dist_lens = limited_lengths(df, maxbits)
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)

        def count(lens, least):
            k = len(lens)
            while k > least and lens[k - 1] == 0:
                k -= 1
            return k

        hlit = count(lit_lens, 257) if hlit is None else hlit
        hdist = count(dist_lens, 1) if hdist is None else hdist
        if not (257 <= hlit <= 288 and 1 <= hdist <= 32):
            raise ValueError('HLIT / HDIST cannot be written')
        seq = (lit_lens + [0] * hlit)[:hlit] + (dist_lens + [0] * hdist)[:hdist]
        if cl_items is None:
            cl_items = run_items(seq)
        cf = [0] * 19
        for it in cl_items:
            cf[it if isinstance(it, int) else it[0]] += 1
        if cl_lens is None:
            cl_lens = limited_lengths(cf, 7)
        k = 19
        while k > 4 and cl_lens[BL_ORDER[k - 1]] == 0:
            k -= 1
        hclen = k if hclen is None else hclen
        p0 = self.bitpos
        self.bits(1 if final else 0, 1)
        self.bits(2, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for j in range(hclen):
            self.bits(cl_lens[BL_ORDER[j]], 3)
        cc = canonical(cl_lens)
        for it in cl_items:
            s = it if isinstance(it, int) else it[0]
            if not cl_lens[s]:
                raise ValueError('code-length symbol %d has no code' % s)
            self.code(cc[s], cl_lens[s])
            if s == 16:
                self.bits(it[1] - 3, 2)
            elif s == 17:
                self.bits(it[1] - 3, 3)
            elif s == 18:
                self.bits(it[1] - 11, 7)
        p1 = self.bitpos
        ntok = self._body(tokens, self._tables(lit_lens), self._tables(dist_lens), eob)
        self._produce(tokens)
        self.shape.append((2, ntok))
        self.block_bits.append((p0, p1, self.bitpos))


def expand(tokens):
    """The bytes a token list produces (no decoder involved).  A distance that reaches before the first byte is a ValueError."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t, (bytes, bytearray)):
            out += t
        elif t[0] == 'raw':
            raise ValueError('a raw symbol produces nothing that can be stated')
        else:
            ln, d = t[0], t[1]
            s = len(out) - d
            if s < 0:
                raise ValueError('distance %d at byte %d' % (d, len(out)))
            if d >= ln:
                out += out[s:s + ln]
            else:
                pat = bytes(out[s:])
                out += (pat * (ln // d + 1))[:ln]
    return bytes(out)


def zwrap(blocks_bits, data=None, cmf=0x78, flg=None, adler=None, trailing=b''):
    """zlib header + the deflate bits (a Writer, or bytes) + adler32 of `data` (default: expand() of the writer's tokens), big-endian.
    flg: the whole FLG byte when given; else FLEVEL 2, no dictionary, FCHECK computed.  adler: the check value when given."""
    w = blocks_bits
    body = w.getvalue() if isinstance(w, Writer) else bytes(w)
    if data is None:
        data = expand(w.tokens)
    if flg is None:
        flg = flg_for(cmf)
    if adler is None:
        adler = zlib.adler32(data) & 0xffffffff
    return bytes([cmf, flg & 0xff]) + body + adler.to_bytes(4, 'big') + trailing


def flg_for(cmf, flevel=2, fdict=0):
    """The FLG byte with FCHECK computed."""
    flg = (flevel << 6) | (fdict << 5)
    return flg + (31 - ((cmf << 8) | flg) % 31) % 31
