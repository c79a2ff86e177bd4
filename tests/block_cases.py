"""Seeded byte streams that drive the block encoder (deflate.hip sections T, L, B) and inflate's dynamic-header decoder to the
edges of zlib's trees.c: length-limited trees with the overflow repair, every kind of run item in a dynamic header, the
extremes of HLIT / HDIST, stored blocks at several bit phases, blocks that end exactly with the token buffer.

Every stream is built for ONE edge and is at most ~100 KB, with three exceptions that need a full block of chosen tokens behind
the blocks it takes to get there: the skewlen cases (286 KB, four blocks: inputs.skewlen starts with 40000 random bytes and its
copies are long), fixed_full_block (~175 KB: two stored blocks, then 16383 tokens with ~2100 matches of every length) and
short_farcopies (~130 KB).  tests/test_block_cases.py checks on the CPU -- against stdlib zlib and the C oracle's report -- that
the cases together reach every item of its checklist, tests/test_gpu_block_edges.py runs them on the device.
"""
import functools
import zlib

import numpy as np

from tests import inputs
from tests.deflate_shape import DIST_BASE

LEVELS = (1, 6, 9)


DB = DIST_BASE + (32769,)          # base distance of every distance code, and the end of the last one's range


def _rng(seed):
    return np.random.RandomState(seed)


def _words(r, n):
    return [bytes(w) for w in r.randint(0, 256, size=(n, 4)).astype(np.uint8)]


def dist_stairs(seed, ratio, ncode, first):
    """4-byte slots; distance code first + i is used round(ratio ** i) times, the rarest codes are the nearest: the distance
    tree comes out higher than 15 and zlib's overflow repair runs on it (nothing else in the suite does that).
    A slot that wants code c repeats the word 4 k bytes back, 4 k inside the code's distance range, if that word has not
    occurred since and k is not the slot before's k (else the match would be found nearer, or grow past 4 bytes)."""
    r = _rng(seed)
    n0 = DB[first + ncode] // 4 + 2
    slots = _words(r, n0)
    last = {w: i for i, w in enumerate(slots)}
    want = np.repeat(np.arange(ncode), [int(round(ratio ** i)) for i in range(ncode)])
    r.shuffle(want)
    prev_k = 0
    for c in want:
        c = first + int(c)
        lo, hi = DB[c], DB[c + 1] - 1                  # the code's distances, in bytes
        klo, khi = (lo + 3) // 4, hi // 4
        i = len(slots)
        w = None
        for _ in range(50):
            k = int(r.randint(klo, khi + 1))
            cand = slots[i - k]
            if last[cand] == i - k and k != prev_k:
                w, prev_k = cand, k
                break
        if w is None:
            w, prev_k = _words(r, 1)[0], 0
        slots.append(w)
        last[w] = i
    return b''.join(slots)


def gap(R, n=4000, seed=0):
    """Two byte values, 0 and R + 1 (0 and 255 for R = 254): the run of zero code lengths between the two literals is exactly R,
    the one from R + 2 to 255 is 254 - R."""
    r = _rng(1000 + R + seed)
    hi = 255 if R == 254 else R + 1
    return (r.randint(0, 2, size=n) * hi).astype(np.uint8).tobytes()


GAP_R = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 137, 138, 139, 140, 141, 148, 149, 150, 200, 254)


def equal_run(K, reps=400, seed=0):
    """K consecutive byte values with equal counts (concatenated random permutations): K equal nonzero code lengths in a row,
    or two runs of neighbouring lengths, on both sides of the 7 / 6 grouping of code 16."""
    r = _rng(2000 + K + seed)
    return np.concatenate([r.permutation(K) for _ in range(reps)]).astype(np.uint8).tobytes()


EQUAL_K = (3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 19, 20)


def literal_only(n, seed):
    """200 symbols with weights 1.03 ** i, a byte skipped whenever it would complete a trigram already seen: no match anywhere,
    one dynamic block with HLIT = 257 and the two forced distance codes."""
    r = _rng(seed)
    p = 1.03 ** np.arange(200)
    p /= p.sum()
    out = bytearray()
    seen = set()
    while len(out) < n:
        for b in r.choice(200, size=4096, p=p):
            b = int(b)
            if len(out) >= 2:
                t = (out[-2], out[-1], b)
                if t in seen:
                    continue
                seen.add(t)
            out.append(b)
            if len(out) == n:
                break
    return bytes(out)


def jitter(n, pattern, seed=0):
    """Byte b has weight pattern[b % len(pattern)]: neighbouring code lengths differ, almost nothing in the header is a run, so
    the header is as long as zlib makes them."""
    r = _rng(3000 + seed)
    p = np.array([pattern[b % len(pattern)] for b in range(256)], dtype=np.float64)
    p /= p.sum()
    return r.choice(256, size=n, p=p).astype(np.uint8).tobytes()


def stored_between(k):
    """Text, then 40000 uniform random bytes, then text: stored blocks behind a dynamic block that ends at a bit phase which
    depends on k."""
    r = _rng(4000 + k)
    return inputs.textlike(5000 + 37 * k, k) + r.randint(0, 256, size=40000).astype(np.uint8).tobytes() + inputs.textlike(3000, k + 9)


def all_matches(ntok, seed=0, nwords=160):
    """Exactly `ntok` tokens at every level, and all of them matches except the 4 * nwords literals no stream can do without:
    `nwords` random 4-byte words with distinct first bytes (and hash chains of their own), then one 4-byte slot per token that repeats one of the words.  A
    slot's word never follows the same word twice, so no match grows to 5 bytes and none starts inside a slot: greedy and lazy
    parses are the same ntok - 4 * nwords matches of length 4, and the token buffer fills up (16383) on a match."""
    r = _rng(5000 + seed)
    words, taken, firsts = [], set(), set()
    while len(words) < nwords:
        w = bytes(r.randint(0, 256, size=4).astype(np.uint8))
        # zlib's hash of the two trigrams every occurrence of the word has: two words in one hash chain would use up the four
        # candidates level 1 looks at
        h = {((w[k] << 10) ^ (w[k + 1] << 5) ^ w[k + 2]) & 0x7fff for k in (0, 1)}
        if w[0] in firsts or len(h) < 2 or h & taken:
            continue
        firsts.add(w[0])
        taken |= h
        words.append(w)
    seq = list(range(nwords))
    used = set(zip(seq, seq[1:]))
    last = {w: i for i, w in enumerate(seq)}
    while len(seq) < ntok - 3 * nwords:
        i = len(seq)
        while True:
            w = int(r.randint(1, nwords))               # (not word 0: zlib never matches position 0)
            if (seq[-1], w) not in used and 4 * (i - last[w]) < 32000:
                break
        used.add((seq[-1], w))
        last[w] = i
        seq.append(w)
    return b''.join(words[w] for w in seq)


def short_farcopies(seed, ntok=16383):
    """Copies of 4 .. 8 bytes from 16 .. 32 KiB back in random data: ~18 bits a token (13 of them distance extra bits), so a
    full block is larger than the 8192-word image the pack kernel assembles a block in and spills into the output directly."""
    r = _rng(6000 + seed)
    out = bytearray(r.randint(0, 256, size=2 * 16383 + 300).astype(np.uint8).tobytes())
    for _ in range(ntok + 200):
        s = len(out) - int(r.randint(16385, 32000))
        out += out[s:s + int(r.randint(4, 9))]
    return bytes(out)


_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
MAX_DIST = 32506

# How often each literal/length symbol and each distance code occurs in fixed_full_block's 16383 tokens.  Every symbol the fixed
# code gives 7 or 8 bits occurs ~72 times, every 9-bit literal ~35 times, the distance codes about equally often: the dynamic
# trees then save ~430 bits on the tokens, but with so many equal counts zlib's tie-breaking scatters 7- and 8-bit lengths
# through the header, which costs more than that.  The counts were moved by 1 .. 8 at a time by a hill climb on a Python port of
# trees.c's build_tree / scan_tree costs until static_len - opt_len was -79.
FIXED_BLOCK_LCOUNTS = (
    72, 68, 71, 72, 72, 71, 72, 69, 72, 70, 72, 71, 70, 72, 72, 72, 72, 72, 72, 72, 72, 70, 71, 72, 71, 70, 71, 71, 72, 72,
    71, 71, 72, 73, 72, 72, 70, 74, 72, 71, 69, 73, 72, 72, 72, 75, 68, 71, 70, 74, 72, 72, 69, 71, 72, 72, 72, 72, 72, 71,
    72, 72, 72, 72, 72, 72, 72, 72, 71, 72, 71, 71, 72, 72, 68, 72, 72, 73, 72, 72, 69, 70, 72, 71, 72, 72, 72, 72, 73, 72,
    72, 69, 73, 70, 72, 72, 71, 74, 71, 72, 69, 72, 72, 72, 72, 70, 71, 71, 71, 72, 72, 72, 71, 70, 72, 72, 72, 72, 72, 71,
    72, 72, 72, 72, 70, 70, 72, 68, 72, 72, 72, 70, 68, 71, 72, 72, 72, 72, 70, 72, 70, 70, 72, 69, 33, 35, 34, 36, 35, 35,
    36, 35, 33, 36, 34, 33, 36, 35, 35, 40, 35, 35, 36, 34, 35, 35, 35, 36, 35, 34, 34, 36, 35, 35, 35, 35, 36, 34, 35, 33,
    37, 34, 35, 35, 38, 35, 35, 37, 35, 35, 35, 33, 35, 34, 35, 33, 34, 34, 36, 36, 35, 35, 35, 38, 35, 33, 37, 35, 34, 35,
    37, 35, 35, 36, 35, 35, 33, 35, 35, 35, 36, 36, 34, 35, 35, 36, 35, 35, 36, 35, 35, 37, 35, 35, 36, 35, 35, 38, 35, 34,
    36, 35, 36, 36, 35, 34, 35, 35, 36, 36, 38, 36, 34, 38, 35, 35, 1, 72, 72, 72, 96, 72, 72, 72, 72, 88, 72, 72, 72, 72,
    96, 72, 72, 72, 80, 83, 72, 72, 72, 72, 70, 63, 72, 71, 71, 72)
FIXED_BLOCK_DCOUNTS = (
    70, 74, 70, 71, 74, 72, 74, 72, 68, 73, 72, 63, 72, 73, 74, 72, 74, 73, 74, 74, 72, 74, 74, 64, 71, 71, 74, 72, 74, 73)


def fixed_full_block(seed=0):
    """A full block (16383 tokens) that zlib level 9 writes with the FIXED codes and that is not the last one: two blocks of random
    literals (stored), the tokens of FIXED_BLOCK_LCOUNTS / _DCOUNTS, then text.  The stored / fixed / dynamic decision is taken
    with the sizes ten bytes apart, HLIT = 286 and HDIST = 30 in the trees that lose, and a block follows at whatever bit phase
    the fixed one ends.  The counts only decide if zlib parses exactly the tokens meant, so the stream is built token by token:
    a literal never completes a trigram seen before (no match can start there), a match's string occurs nowhere else in the
    window, nor does what the lazy step looks at one byte later, the byte behind a match is not the one that would make it
    longer, and a match of 3 bytes gets a distance of at most 4096 (zlib drops a farther one)."""
    r = _rng(9000 + seed)
    out = bytearray()
    seen = set()                      # every trigram of `out`

    def push(bs):
        for b in bs:
            out.append(b)
            if len(out) >= 3:
                seen.add(bytes(out[-3:]))
    # two blocks of literals: random bytes, none completing a trigram that occurred before (no match anywhere)
    while len(out) < 2 * 16383:
        b = int(r.randint(256))
        if len(out) >= 2 and bytes(out[-2:]) + bytes([b]) in seen:
            continue
        push([b])
    # the tokens: every literal/length symbol as often as wanted, every match with a distance code (a match of 3 bytes with one
    # of at most 4096: zlib drops such a match when it is farther)
    syms = np.repeat(np.arange(286), FIXED_BLOCK_LCOUNTS)
    syms = syms[syms != 256]
    dcs = np.repeat(np.arange(30), FIXED_BLOCK_DCOUNTS)
    r.shuffle(dcs)
    dcs = sorted(dcs.tolist(), key=lambda c: c >= 24)            # (stable: the near codes first, in random order)
    m3 = int((syms == 257).sum())
    near, rest = dcs[:m3], dcs[m3:]
    r.shuffle(rest)
    pool = [(int(s), -1) for s in syms if s < 256] + [(257, c) for c in near] + \
           [(int(s), c) for s, c in zip(syms[syms > 257], rest)]
    order = r.permutation(len(pool))
    pool = [pool[i] for i in order]
    nlit = 2                          # how many of the last positions are literal tokens (at most 2 matter)
    ext = None                        # the byte that would make the match before one longer
    ntok = 0
    while pool and ntok < 16383:
        done = False
        for attempt in range(300):
            j = int(r.randint(len(pool))) if attempt else len(pool) - 1
            s, dc = pool[j]
            if s < 256:
                bs = bytes([s])
            else:
                L = _LEN_BASE[s - 257]
                d = int(r.randint(DB[dc], min(DB[dc + 1] - 1, MAX_DIST) + 1))
                src = len(out) - d
                tmp = bytearray(out[src:src + L])
                while len(tmp) < L:
                    tmp.append(tmp[len(tmp) - d])
                bs = bytes(tmp)
            if bs[0] == ext:
                continue
            # a literal position must start no trigram that occurred before
            tail = bytes(out[-2:]) + bs[:2]
            if nlit >= 2 and tail[0:3] in seen and len(tail) >= 3:
                continue
            if nlit >= 1 and len(tail) >= 4 and tail[1:4] in seen:
                continue
            if s >= 256:
                # the string (and what the lazy step looks at one position later) occurs nowhere else in the window
                w0 = max(0, len(out) - MAX_DIST)
                hay = bytes(out[w0:]) + bs
                p = hay.find(bs)
                if p != src - w0 or hay.find(bs, p + 1) != len(out) - w0:
                    continue
                if L > 3:
                    t = bs[1:]
                    p = hay.find(t)
                    if d < L:                     # an overlapping copy: the other places are shifts inside the run itself
                        if p < src - w0:
                            continue
                    elif p != src + 1 - w0 or hay.find(t, p + 1) != len(out) + 1 - w0:
                        continue
            # a literal after one literal: trigram (prev lit, this, next) is checked when the next token comes
            if s < 256:
                push(bs); nlit = min(nlit + 1, 2); ext = None
            else:
                push(bs); nlit = 0
                ext = out[src + L] if L < 258 else None
            pool[j] = pool[-1]; pool.pop()
            ntok += 1
            done = True
            break
        if not done:
            pool.pop()                # (cannot be placed: the count is one short, and test_block_cases.py sees what zlib makes of it)
    return bytes(out) + inputs.textlike(3000, seed)


# Literal/length overflow: inputs.skewlen as it is (overflow 6 in its fourth block) and two more settings of (seed, ratio, nsym,
# nlen), picked from a scan of ratio 1.55 .. 1.7 x nsym 20 .. 40 x seeds 6 .. 8 on the CPU (zlib level 6): overflow 2, 4, 6, 8,
# 10, 12 and 14 all occur; these three give 6, 14 and 2.  The stream is cut behind the fourth block (the first three are what it
# takes to get past the generator's 40000 random bytes).
SKEWLEN = ((6, 1.65, 22, 8), (8, 1.66, 24, 8), (7, 1.68, 24, 8))
SKEWLEN_BYTES = 286000


@functools.lru_cache(maxsize=None)
def cases():
    """name -> bytes, in a fixed order (the batched GPU test puts them into one call in this order)."""
    c = {}
    for seed in (0, 1):
        c['dist_stairs_1.7_17_13_s%d' % seed] = dist_stairs(seed, 1.7, 17, 13)
        c['dist_stairs_1.66_18_12_s%d' % seed] = dist_stairs(seed, 1.66, 18, 12)
    for R in GAP_R:
        c['gap_%d' % R] = gap(R)
    for K in EQUAL_K:
        c['equal_run_%d' % K] = equal_run(K)
    for n in (600, 3000, 20000):
        c['literal_only_%d' % n] = literal_only(n, n)
    for pat in ((1, 3, 9, 27), (1, 2, 4, 8, 16, 32)):
        for n in (12000, 16000):
            c['jitter_%d_%s' % (n, 'x'.join(map(str, pat)))] = jitter(n, pat)
    for k in range(12):
        c['stored_between_%d' % k] = stored_between(k)
    for seed, ratio, nsym, nlen in SKEWLEN:
        c['skewlen_%g_%d_%d_s%d' % (ratio, nsym, nlen, seed)] = inputs.skewlen(SKEWLEN_BYTES, seed, ratio, nsym, nlen)
    for T in (16382, 16383, 16384):
        c['all_matches_%d' % T] = all_matches(T)
    c['short_farcopies'] = short_farcopies(0)
    c['fixed_full_block'] = fixed_full_block(0)
    c['stored_last'] = inputs.textlike(3000, 1) + _rng(8000).randint(0, 256, size=30000).astype(np.uint8).tobytes()
    c['empty'] = b''
    c['one_byte'] = b'\x5a'
    return c


# ------------------------------------------------------------------------------------------------
# what zlib and the oracle say about a case (computed once per process, shared by the tests)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zbytes(name, level):
    return zlib.compress(cases()[name], level)


@functools.lru_cache(maxsize=None)
def shape(name, level):
    """deflate_shape.blocks() of zlib's stream."""
    from tests import deflate_shape
    return deflate_shape.blocks(zbytes(name, level))


@functools.lru_cache(maxsize=None)
def oracle_report(name, level):
    """(stream, tokens, block reports) of the C oracle."""
    from oracle import oracle as O
    z, toks, _, blocks = O.deflate(cases()[name], level, report=True)
    return z, toks, blocks


def describe_block(name, level, i):
    """One line on block i of a case: what a failure report needs to say where a wrong byte lies."""
    b, o = shape(name, level)[i], oracle_report(name, level)[2][i]
    s = 'block %d: btype %d%s, bits [%d, %d), %d tokens, overflow l/d/bl %d/%d/%d' % (
        i, b['btype'], ' (last)' if b['last'] else '', b['bit_start'], b['bit_end'], o['ntok'], o['ovf_l'], o['ovf_d'], o['ovf_bl'])
    if b['btype'] == 0:
        s += ', %d padding bits, LEN %d' % (b['pad'], b['len'])
    if b['btype'] == 2:
        s += ', HLIT %d HDIST %d HCLEN %d, header %d bits, longest codes l/d/bl %d/%d/%d, items %s' % (
            b['hlit'], b['hdist'], b['hclen'], b['hdr_bits'], b['l_max_len'], b['d_max_len'], b['bl_max'], b['items'])
    return s
