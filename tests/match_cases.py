"""Seeded byte streams that put the match finder (match.hip: k_match5 / k_match6) and the lazy parse (deflate.hip) on the exact
off-by-one rules of zlib's longest_match / deflate_slow and on the boundaries of the kernels' own geometry.

Every case is built for ONE rule, names it in its docstring, and comes with a certificate: a function of the level that returns
counts, computed from the oracle's traced walk (oracle.match_trace), from a re-walk of the tables (parse_events) or from the
sorted order of a tile (geometry), that prove the stream reaches the rule.  tests/test_match_cases.py asserts on the CPU that
every count is at least 1 at every level the case claims; tests/test_gpu_match_edges.py holds the device to the oracle on them.
Nothing here touches the device.

Streams are random filler (cheap for the oracle: chains of one or two) around the planted region, at most ~270 KB.
"""
import functools
import zlib

import numpy as np

# the geometry the kernels share with the host plan (mtscomp_amd/csrc/codec_plan.h, match.hip)
TILE, HALO = 229376, 32768
MAX_DIST, TOO_FAR = 32506, 4096
M5_WAVES, M5_SLICES, M6_SLICES, M6_WG_THREADS = 8, 64, 64, 512
ALL = (4, 5, 6, 7, 8, 9)
CFG = {4: (16, 4, 4, 16), 5: (32, 8, 16, 32), 6: (128, 8, 16, 128), 7: (256, 8, 32, 128), 8: (1024, 32, 128, 258),
       9: (4096, 32, 258, 258)}          # level -> chain, good, lazy, nice
MAX_INSERT = {1: 4, 2: 5, 3: 6}
END_NONE, END_NICE, END_BUDGET, END_LIMIT, END_CHAIN = range(5)


def hash3(b0, b1, b2):
    return ((b0 << 10) ^ (b1 << 5) ^ b2) & 0x7fff


def hashes(a):
    a = np.asarray(a, dtype=np.uint8).astype(np.int64)
    return ((a[:-2] << 10) ^ (a[1:-1] << 5) ^ a[2:]) & 0x7fff


def trigram_of_hash(r, h):
    """Three random bytes whose hash is h."""
    b2 = (h & 31) | int(r.randint(8)) << 5; hi = int(r.randint(8)); b0hi = int(r.randint(8))
    x = h ^ b2
    b1 = ((x >> 5) & 31) | (hi << 5)
    b0 = (((x >> 10) & 31) ^ hi) | (b0hi << 5)
    assert hash3(b0, b1, b2) == h
    return bytes((b0, b1, b2))


# ------------------------------------------------------------------------------------------------
# geometry: where the kernels put a position
# ------------------------------------------------------------------------------------------------
def tiles_of(n):
    """(a, w, wlen, own_end) of every match-stage tile of an n-byte chunk (CompressPlan)."""
    out = []
    for a in range(0, n, TILE):
        w = max(0, a - HALO)
        own_end = min(a + TILE, n)
        hashed_end = (min(own_end, n - 2) if n >= 3 else 0)
        out.append((a, w, max(0, hashed_end - w), own_end))
    return out


def sorted_window(data, tile):
    """The tile's sorted order: positions of its window by (hash, position)."""
    a, w, wlen, _ = tile
    if wlen == 0:
        return np.zeros(0, np.int64)
    h = hashes(np.frombuffer(data, np.uint8)[w:w + wlen + 2])
    return np.argsort(h, kind='stable') + w


def m5_groups_per_wave(wlen, nsl=M5_SLICES):
    ng = (wlen + 63) // 64
    return (ng + nsl * M5_WAVES - 1) // (nsl * M5_WAVES)


def m6_groups_per_workgroup(wlen, nsl=M6_SLICES):
    ng = (wlen + 63) // 64
    return ((ng + nsl - 1) // nsl + M5_WAVES - 1) // M5_WAVES * M5_WAVES


def locate(data, p):
    """Tile, slot, group and lane of the position that owns table entry p -- for failure messages."""
    for t, tile in enumerate(tiles_of(len(data))):
        if tile[0] <= p < tile[3]:
            s = np.nonzero(sorted_window(data, tile) == p)[0]
            if not s.size:
                return 'tile %d, not hashed' % t
            s = int(s[0])
            return 'tile %d, slot %d, group %d, lane %d' % (t, s, s // 64, s % 64)
    return 'no tile'


def run_slots(data, tile, h):
    """[first, last + 1) slot of hash h in the tile's sorted order."""
    a, w, wlen, _ = tile
    hs = hashes(np.frombuffer(data, np.uint8)[w:w + wlen + 2])
    start = int((hs < h).sum())
    return start, start + int((hs == h).sum())


# ------------------------------------------------------------------------------------------------
# building
# ------------------------------------------------------------------------------------------------
class Plan:
    """Random filler with planted strings; scrub() then takes a hash away from every position that was not planted with it."""

    def __init__(self, n, seed):
        self.r = np.random.RandomState(seed)
        self.buf = self.r.randint(0, 256, size=n).astype(np.uint8)
        self.prot = np.zeros(n, bool)

    def put(self, pos, bs):
        bs = np.frombuffer(bytes(bs), np.uint8)
        assert pos >= 0 and pos + bs.size <= self.buf.size and not self.prot[pos:pos + bs.size].any(), pos
        self.buf[pos:pos + bs.size] = bs
        self.prot[pos:pos + bs.size] = True

    def rand(self, k):
        return self.r.randint(0, 256, size=k).astype(np.uint8).tobytes()

    def other(self, byte):
        return bytes(((int(byte) + 1 + int(self.r.randint(255))) & 255,))

    def scrub(self, owned):
        """owned: hash -> positions allowed to have it."""
        for _ in range(50):
            hs = hashes(self.buf)
            dirty = False
            for h, pos in owned.items():
                bad = np.setdiff1d(np.nonzero(hs == h)[0], np.asarray(sorted(pos)))
                for p in bad:
                    free = [q for q in (p + 2, p + 1, p) if not self.prot[q]]
                    assert free, ('a planted string has the hash of another', h, int(p))
                    self.buf[free[0]] ^= 1 + int(self.r.randint(31))
                    dirty = True
            if not dirty:
                return
        raise AssertionError('scrub does not converge')

    def bytes(self):
        return self.buf.tobytes()


class Case:
    def __init__(self, name, doc, data, cert, levels=ALL, marks=None):
        self.name, self.doc, self.data, self.cert, self.levels, self.marks = name, doc, data, cert, levels, marks or {}


def _len(v):
    return int(v) >> 16


def _dist(v):
    return int(v) & 0xffff


# ---- budget -------------------------------------------------------------------------------------
BACKS = sorted({b for c, _, _, _ in CFG.values() for b in (c, c + 1, c // 4, c // 4 + 1)})


def plant_budget_run(pl, s0_pos, spacing=6):
    """One hash run of 6-byte strings T x y z.  For every b in BACKS one target string whose only equal x y z lies exactly b
    strings back; every string in between has another x (it fails at byte 3 and must still count).  The first target is the
    string at s0_pos, every source lies before it.  Returns ({b: target position}, T, positions of the run)."""
    T = pl.rand(3)
    first = -(max(BACKS) + 8)
    used, plan = set(), {}
    t = 0
    for b in BACKS:
        while t in used or (t - b) in used or t - b >= 0:
            t += 1
            assert t < b
        used |= {t, t - b}
        plan[b] = t
        t = 0
    last = max(plan.values()) + 2
    tails = {}
    for k, (b, t) in enumerate(plan.items()):
        tails[t] = tails[t - b] = bytes((200 + k,)) + pl.rand(2)
    pos = []
    for i in range(first, last + 1):
        tail = tails.get(i) or bytes((int(pl.r.randint(200)),)) + pl.rand(2)
        pl.put(s0_pos + spacing * i, T + tail)
        pos.append(s0_pos + spacing * i)
    return {b: s0_pos + spacing * t for b, t in plan.items()}, T, pos


def budget_cert(marks):
    def cert(level, tr):
        c = CFG[level][0]
        q = c // 4
        f, g, qf, qg = marks[c], marks[c + 1], marks[q], marks[q + 1]
        return {
            'winner is candidate number chain': int(tr['full_idx'][f] == c and tr['end'][f] == END_BUDGET and _len(tr['t_full'][f]) > 3),
            'candidates before it fail at byte 3 and count': int(tr['fail3'][f] >= c - 1 and tr['visited'][f] == c),
            'longest is candidate chain + 1: missed': int(tr['end'][g] == END_BUDGET and tr['visited'][g] == c and
                                                          tr['beyond_len'][g] > _len(tr['t_full'][g]) == 3),
            'quarter winner is candidate number chain / 4': int(tr['quarter_idx'][qf] == q and _len(tr['t_quarter'][qf]) > 3),
            'quarter misses candidate chain / 4 + 1': int(tr['quarter_missed'][qg] == 1 and tr['t_quarter'][qg] != tr['t_full'][qg]
                                                          and tr['full_idx'][qg] == q + 1),
        }
    return cert


def budget():
    """Chain budget: per level, the longest candidate is number `chain` of its run (taken) and, for a sibling, number chain + 1
    (missed: a 3-byte match wins); the same at chain / 4 for the quarter result.  Everything in between fails at byte 3."""
    pl = Plan(36000, 11)
    s0 = 4000 + 6 * (max(BACKS) + 8)
    marks, T, pos = plant_budget_run(pl, s0)
    pl.scrub({hash3(*T): pos})
    return Case('budget', budget.__doc__, pl.bytes(), budget_cert(marks), marks=marks)


# ---- runs against the kernel's units ----------------------------------------------------------------
RUN_LENGTHS = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)
RUN_N = 32768          # 512 groups: k_match6's workgroups start every 8 groups, k_match5's waves every group (64 slices) or every 64 (1 slice)
RUN_BOUNDARY = 4096    # slots: a multiple of all of them


def run_case(N):
    """A hash run of N slots in a 32768-byte stream, placed in the sorted order so that it lies on both sides of a slot that
    is a multiple of 4096: a 64-slot group boundary, the first group of a k_match5 wave with 1 and with 64 slices (history
    staged again), and the first group of a k_match6 workgroup (look-back; from 513 slots before it on, a second round)."""
    assert m5_groups_per_wave(RUN_N - 2, 1) == 64 and m5_groups_per_wave(RUN_N - 2, 64) == 1 and m6_groups_per_workgroup(RUN_N - 2) == 8
    want_before = 600 if N >= 1023 else 1
    for attempt in range(4000):
        pl = Plan(RUN_N, 5000 + N)
        r = np.random.RandomState(N * 7919 + attempt)
        h = int(r.randint(1, 0x7fff))
        T = trigram_of_hash(r, h)
        base = 8000
        pos = [base + 4 * i for i in range(N)]
        body = bytearray()
        for i in range(N):
            body += T + bytes((int(r.randint(256)),))
        pl.put(base, bytes(body))
        hs = hashes(pl.buf)
        start = int((hs < h).sum())
        B = (start + N - 1) // RUN_BOUNDARY * RUN_BOUNDARY
        # (the scrub moves a few filler positions to other hashes: a margin of 8 slots on both sides)
        if not (B > 0 and B - start >= want_before + 8 and start + N - B >= 9):
            continue
        try:
            pl.scrub({h: pos})
        except AssertionError:
            continue
        data = pl.bytes()
        a, e = run_slots(data, tiles_of(RUN_N)[0], h)
        if e - a == N and B - a >= want_before and e - B >= 1:
            break
    else:
        raise AssertionError('no placement for a run of %d' % N)

    def cert(level, tr):
        a, e = run_slots(data, tiles_of(RUN_N)[0], h)
        c = CFG[level][0]
        first_after = int(sorted_window(data, tiles_of(RUN_N)[0])[B])
        out = {'run of exactly N slots': int(e - a == N),
               'slots on both sides of a group / wave / workgroup start': int(a < B < e and B % (64 * 64) == 0),
               'the first slot behind it has its chain before it': int(tr['visited'][first_after] == min(B - a, c))}
        if N >= 1023 and c > M6_WG_THREADS:
            out['second look-back round'] = int(B - a > M6_WG_THREADS)
        return out
    return Case('run_%d' % N, run_case.__doc__, data, cert, marks={'hash': h, 'boundary': B})


# ---- hash collisions ------------------------------------------------------------------------------
def collisions():
    """Equal 15-bit hash, different bytes 0..2, one string for each way the hash hides a bit (b0[7:5] not in it; b0[2:0]
    against b1[7:5]; b1[2:0] against b2[7:5]), bytes 3..12 the target's: only the entry's 9 proof bits reject them.  One group
    of nine colliders in front of the true match for every level, and per level a group that puts the true match at chain
    index `chain` behind chain - 1 colliders (7-byte strings for 4096)."""
    pl = Plan(60000, 21)
    r = pl.r
    marks, owned = {}, {}
    at = 200

    def group(ncol, slen, key):
        nonlocal at
        T = bytes(r.randint(8, 248, size=3).astype(np.uint8))
        tail = pl.rand(slen - 3)
        more = pl.rand(8)
        h = hash3(*T)
        pos = [at]
        pl.put(at, b'\x00' + T + tail + more + b'\x01'); at += 1          # (the true match, one byte in: never at position 0)
        pos[0] = at
        at += slen + 8 + 3
        for i in range(ncol):
            k = 1 + i // 3 % 7
            kind = i % 3
            b0, b1, b2 = T
            if kind == 0:
                b0 ^= k << 5
            elif kind == 1:
                b0 ^= k; b1 ^= k << 5
            else:
                b1 ^= k; b2 ^= k << 5
            assert hash3(b0, b1, b2) == h and bytes((b0, b1, b2)) != T
            pl.put(at, bytes((b0, b1, b2)) + tail)
            pos.append(at)
            at += slen
        pl.put(at, T + tail + more + b'\x02')
        pos.append(at)
        marks[key] = (at, ncol)
        at += slen + 8 + 3
        owned[h] = pos
    group(9, 13, 'all')
    for lv in ALL:
        c = CFG[lv][0]
        group(c - 1, 13 if c <= 1024 else 7, lv)
    pl.scrub(owned)

    def cert(level, tr):
        out = {}
        for key in ('all', level):
            p, ncol = marks[key]
            out['%s: colliders visited and counted, the winner behind them' % key] = int(
                tr['collisions'][p] == ncol and tr['full_idx'][p] == ncol + 1 and tr['visited'][p] == ncol + 1 and _len(tr['t_full'][p]) >= 15)
        p, ncol = marks[level]
        out['the winner is candidate number chain'] = int(tr['full_idx'][p] == CFG[level][0])
        out['the quarter result misses it'] = int(tr['t_quarter'][p] == 0)
        return out
    return Case('collisions', collisions.__doc__, pl.bytes(), cert, marks=marks)


# ---- compare-length limits ------------------------------------------------------------------------------
CMP_LENGTHS = tuple(range(3, 22)) + tuple(range(254, 259))


def cmp_len():
    """True match lengths 3..21 and 254..258, source and target at every pair of address phases mod 4, so the differing byte
    sits at every place of the compare's 4-byte step.  Length 7 ends at a byte 7 that differs in its high three bits only (the
    entry holds the low five); 13 and 14 end with the ring of bytes 7..12; one 258-byte match goes on for a 259th byte."""
    r = np.random.RandomState(31)
    out = bytearray(r.randint(0, 256, size=64).astype(np.uint8).tobytes())
    marks = []

    def pad_to(phase):
        while len(out) % 4 != phase:
            out.append(int(r.randint(256)))
    for L in CMP_LENGTHS:
        for pa in range(4):
            for pb in range(4):
                body = r.randint(0, 256, size=L + 1).astype(np.uint8)
                if L == 7:
                    diff = (0x20, 0x40, 0x80, 0xe0)[pb]
                elif L == 258 and (pa + pb) % 2 == 0:
                    diff = 0                                      # the 259th byte matches as well
                else:
                    diff = 1 + int(r.randint(255))
                src = body.copy(); src[L] ^= diff
                pad_to(pa); a = len(out); out += src.tobytes()
                out += r.randint(0, 256, size=5).astype(np.uint8).tobytes()
                pad_to(pb); b = len(out); out += body.tobytes()
                out += r.randint(0, 256, size=3).astype(np.uint8).tobytes()
                marks.append((L, pa, pb, a, b, diff))
    out += r.randint(0, 256, size=300).astype(np.uint8).tobytes()
    data = bytes(out)

    def cert(level, tr):
        ok = {}
        for L, pa, pb, a, b, diff in marks:
            good = int(tr['t_full'][b]) == (L << 16 | (b - a)) and a % 4 == pa and b % 4 == pb
            ok.setdefault(L, []).append(good)
        res = {'length %d at all 16 phase pairs' % L: int(all(v) and len(v) == 16) for L, v in ok.items()}
        res['length 7 ends at a byte that differs in bits 7:5 only'] = sum(1 for m in marks if m[0] == 7 and m[5] & 0x1f == 0)
        res['258 with an equal 259th byte'] = sum(1 for m in marks if m[0] == 258 and m[5] == 0 and data[m[3] + 258] == data[m[4] + 258])
        return res

    def fast_cert(level, toks):
        lens = set((toks[toks[:, 0] != 0, 1] + 3).tolist())
        m = MAX_INSERT[level]
        return {'a match of max_insert_length': int(m in lens), 'a match of max_insert_length + 1': int(m + 1 in lens)}
    c = Case('cmp_len', cmp_len.__doc__, data, cert, marks=marks)
    c.fast_cert = fast_cert
    return c


# ---- nice_match -----------------------------------------------------------------------------------------
def nice():
    """Per nice_match value (16, 32, 128, 258): the newest candidate has length nice - 1, nice and nice + 1 (258: 257 and 258)
    and a longer one is next in the chain.  The longer one is taken only behind nice - 1; at nice the walk ends after one
    candidate."""
    pl = Plan(9000, 41)
    marks, owned = {}, {}
    at = 100
    for v in (16, 32, 128, 258):
        for k in (v - 1, v, v + 1):
            if k > 258:
                continue
            T = pl.rand(3)
            body = pl.rand(min(k + 10, 258) - 3 + 2)
            s2 = at; pl.put(at, T + body + b'\x07'); at += len(body) + 8
            if k < 258:
                newer = T + body[:k - 3] + pl.other(body[k - 3])
            else:
                newer = T + body
            s1 = at; pl.put(at, newer); at += len(newer) + 5
            tg = at; pl.put(at, T + body + b'\x09'); at += len(body) + 9
            marks[(v, k - v)] = tg
            owned[hash3(*T)] = [s2, s1, tg]
    pl.scrub(owned)

    def cert(level, tr):
        v = CFG[level][3]
        m, e = marks[(v, -1)], marks[(v, 0)]
        out = {'behind nice - 1 the longer candidate is taken': int(tr['full_idx'][m] == 2 and _len(tr['t_full'][m]) > v - 1),
               'at nice the walk ends after one candidate': int(tr['end'][e] == END_NICE and tr['visited'][e] == 1 and
                                                                _len(tr['t_full'][e]) == v and tr['beyond_len'][e] >= v)}
        if v < 258:
            p = marks[(v, 1)]
            out['at nice + 1 as well, a longer one behind it'] = int(tr['end'][p] == END_NICE and tr['visited'][p] == 1 and
                                                                     _len(tr['t_full'][p]) == v + 1 and tr['beyond_len'][p] > v + 1)
        return out
    return Case('nice', nice.__doc__, pl.bytes(), cert, marks=marks)


# ---- distance limits ----------------------------------------------------------------------------------------
def dist_limits():
    """MAX_DIST is 32506 for the chain head and one less for the rest: a head at 32506 is kept, at 32507 dropped; a second
    candidate at exactly 32506 is dropped (the walk ends by the limit with budget left and a longer match just beyond) and at
    32505 kept.  Position 0 is NIL: never a candidate, and a chain through it ends there."""
    pl = Plan(33600, 51)
    owned, marks = {}, {}

    def pair(key, src, dist, mid=None):
        T = pl.rand(3); body = pl.rand(12)
        pos = [src]
        pl.put(src, T + body + b'\x03')
        if mid is not None:
            pl.put(mid, T + pl.other(body[0])); pos.append(mid)
        pl.put(src + dist, T + body + b'\x04'); pos.append(src + dist)
        marks[key] = src + dist
        owned[hash3(*T)] = pos
    pair('head at MAX_DIST', 100, MAX_DIST)
    pair('head at MAX_DIST + 1', 140, MAX_DIST + 1)
    pair('second at MAX_DIST', 180, MAX_DIST, 180 + 900)
    pair('second at MAX_DIST - 1', 220, MAX_DIST - 1, 220 + 900)
    pair('chain through 0', 0, 20000, 5000)
    marks['head is 0'] = 5000
    pl.scrub(owned)
    data = pl.bytes()

    def cert(level, tr):
        a, b, c, d, z, m = (marks[k] for k in ('head at MAX_DIST', 'head at MAX_DIST + 1', 'second at MAX_DIST', 'second at MAX_DIST - 1',
                                               'chain through 0', 'head is 0'))
        return {'head at MAX_DIST kept': int(tr['t_full'][a] == (15 << 16 | MAX_DIST) and tr['head_dist'][a] == MAX_DIST),
                'head at MAX_DIST + 1 dropped': int(tr['t_full'][b] == 0 and tr['head_dist'][b] == MAX_DIST + 1 and tr['end'][b] == END_NONE),
                'second candidate at MAX_DIST dropped, budget left, longer beyond': int(
                    tr['end'][c] == END_LIMIT and tr['visited'][c] == 1 < CFG[level][0] and _len(tr['t_full'][c]) == 3 and tr['beyond_len'][c] == 15),
                'second candidate at MAX_DIST - 1 kept': int(tr['full_idx'][d] == 2 and tr['t_full'][d] == (15 << 16 | (MAX_DIST - 1))),
                'chain ends at position 0, which would be longer': int(tr['end'][z] == END_CHAIN and tr['visited'][z] == 1 and
                                                                       _len(tr['t_full'][z]) == 3 and tr['beyond_len'][z] == 15),
                'position 0 as chain head is no candidate': int(tr['t_full'][m] == 0 and tr['end'][m] == END_NONE and data[m:m + 3] == data[0:3])}
    return Case('dist_limits', dist_limits.__doc__, data, cert, marks=marks)


# ---- parse thresholds -----------------------------------------------------------------------------------------
def parse_events(data, level, tf, tq):
    """deflate_slow on the tables (orc_parse_tables), saying at every lazy step what it read and whether the other table
    would have decided otherwise.  Returns (tokens as (pos, len, dist) with len 0 for literals, list of events)."""
    _, good, lazy, _ = CFG[level]
    n = len(data)
    toks, ev = [], []
    p = 0
    while p < n:
        ln, d = _len(tf[p]), _dist(tf[p])
        too_far = ln == 3 and d > TOO_FAR
        if too_far:
            ev.append(('too_far', p, ln, d)); ln = 0
        if ln < 3:
            toks.append((p, 0, 0)); p += 1
            continue
        defer = 0
        while True:
            q = p + 1
            better = None
            if q < n and ln < lazy:
                use_q = ln >= good
                t = tq[q] if use_q else tf[q]
                o = tf[q] if use_q else tq[q]
                if _len(t) > ln:
                    better = (_len(t), _dist(t))
                obetter = (_len(o), _dist(o)) if _len(o) > ln else None
                ev.append(('lazy', p, ln, 'quarter' if use_q else 'full', int(tq[q] != tf[q]), _len(tq[q]), int(better != obetter)))
            elif q < n:
                ev.append(('held', p, ln, int(_len(tf[q]) > ln)))
            if better is None:
                break
            toks.append((p, 0, 0)); p = q; ln, d = better; defer += 1
        if defer:
            ev.append(('chain', p, defer))
        toks.append((p, ln, d)); p += ln
    return toks, ev


def parse_case(level):
    """Lazy-parse thresholds of one level: a held match of good - 1 (reads t_full) and of good (reads t_quarter) where the two
    differ at the next position, with a quarter length at most good (what the table encodes as QNONE) and of good + 1 (QSIDE),
    and the token changes; held lengths lazy - 1 (looks) and lazy (does not); a 3-byte match at distance 4096 (kept) and 4097
    (a literal); a chain of three deferrals (levels 5..9)."""
    chain, good, lazy, _ = CFG[level]
    q = chain // 4
    pl = Plan(16000 + 6 * q * 3, 60 + level)
    owned = {}
    at = 50

    def put(bs):
        nonlocal at
        pl.put(at, bs); p = at; at += len(bs) + 3
        return p

    def held_then_quarter(held, side):
        """position p holds `held` bytes; at p + 1 the long match (good + 6) is candidate q + 1 behind q fillers of 3 bytes
        (side: the newest of them has good + 1)"""
        M = good + 6
        W = pl.rand(M + 8)
        put(pl.other(W[0]) + W[:held] + pl.other(W[held]))
        put(pl.other(W[0]) + W[1:1 + M] + pl.other(W[1 + M]))
        for j in range(q):
            if side and j == q - 1:
                put(pl.other(W[0]) + W[1:good + 2] + pl.other(W[good + 2]))
            else:
                put(W[1:4] + pl.other(W[4]))
        return put(W + b'\x05')

    marks = {'qnone': held_then_quarter(good, False), 'qside': held_then_quarter(good, True), 'good-1': held_then_quarter(max(good - 1, 3), False)}
    for k in (lazy - 1, lazy):
        W = pl.rand(min(k + 6, 259) + 2)
        put(pl.other(W[0]) + W[:k] + (pl.other(W[k]) if k < len(W) else b''))
        put(pl.other(W[0]) + W[1:min(k + 4, 259)] + b'\x06')
        marks['lazy%+d' % (k - lazy)] = put(W + b'\x05')
    if level >= 5:
        W = pl.rand(16)
        for k in range(4):
            put(pl.other(W[k - 1] if k else 0) + W[k:2 * k + 3] + pl.other(W[2 * k + 3]))
        marks['chain3'] = put(W + b'\x05')
    # a 3-byte match at 4096 and at 4097
    for key, dd in (('4096', TOO_FAR), ('4097', TOO_FAR + 1)):
        T = pl.rand(3); x = pl.rand(1)
        s = put(T + x)
        pl.put(s + dd, T + pl.other(x[0]))
        marks[key] = s + dd
        owned[hash3(*T)] = [s, s + dd]
    pl.scrub(owned)
    data = pl.bytes()

    def cert(lv, tr):
        assert lv == level
        toks, ev = parse_events(data, level, tr['t_full'], tr['t_quarter'])
        lz = {e[1]: e for e in ev if e[0] == 'lazy'}
        held = {e[1]: e for e in ev if e[0] == 'held'}
        tk = {t[0]: t for t in toks}
        a, b, c = lz.get(marks['qnone']), lz.get(marks['qside']), lz.get(marks['good-1'])
        out = {
            'held good reads a quarter result of at most good that differs; the token changes': int(
                a is not None and a[2] == good and a[3] == 'quarter' and a[4] == 1 and a[5] <= good and a[6] == 1),
            'held good reads a quarter result of good + 1 that differs; the token changes': int(
                b is not None and b[2] == good and b[3] == 'quarter' and b[4] == 1 and b[5] == good + 1 and b[6] == 1),
            'held lazy - 1 looks and defers': int(marks['lazy-1'] in lz and lz[marks['lazy-1']][2] == lazy - 1 and (marks['lazy-1'] + 1) in tk
                                                 and tk[marks['lazy-1'] + 1][1] > lazy - 1),
            'held lazy does not look': int(marks['lazy+0'] in held and held[marks['lazy+0']][2] == lazy and tk.get(marks['lazy+0'], (0, 0, 0))[1] == lazy),
            '3 bytes at 4096 kept': int(tk.get(marks['4096']) == (marks['4096'], 3, 4096)),
            '3 bytes at 4097 a literal': int(('too_far', marks['4097'], 3, 4097) in ev and tk[marks['4097']][1] == 0),
        }
        if good >= lazy:      # level 4: a held match of good bytes is one of max_lazy bytes -- the quarter result is never read
            del out['held good reads a quarter result of at most good that differs; the token changes']
            del out['held good reads a quarter result of good + 1 that differs; the token changes']
            out['held good = max_lazy: no quarter result is ever read'] = int(
                not any(e[0] == 'lazy' and e[3] == 'quarter' for e in ev) and marks['qnone'] in held and marks['qside'] in held)
        out['held good - 1 reads t_full where the quarter differs'] = int(c is not None and c[2] == good - 1 and c[3] == 'full' and c[4] == 1)
        if lazy < 258:
            out['held lazy passes a longer match by'] = int(held[marks['lazy+0']][3] == 1) if marks['lazy+0'] in held else 0
        if level >= 5:
            out['three deferrals in a row'] = int(any(e[0] == 'chain' and e[2] >= 3 for e in ev))
        return out
    return Case('parse_L%d' % level, parse_case.__doc__, data, cert, levels=(level,), marks=marks)


# ---- end of chunk -------------------------------------------------------------------------------------------------
def tail_case(n):
    """A 7-byte period behind one odd byte, n bytes in all (n = 3, 4, 5: one byte value): every match runs into the last byte,
    the lookahead clips nice_match and the match length, position n - 3 has exactly three bytes."""
    r = np.random.RandomState(70 + n)
    if n <= 5:
        data = bytes((0x41,)) * n
    else:
        ph = r.randint(0, 256, size=7).astype(np.uint8).tobytes()
        data = (b'\xff' + ph * (n // 7 + 2))[:n]

    def cert(level, tr):
        out = {'hashed positions': max(n - 2, 0)}
        if n >= 5:
            out['a match at the position with exactly three bytes'] = int(_len(tr['t_full'][n - 3]) == 3)
        if n >= 257:
            ln = np.array([_len(v) for v in tr['t_full']])
            p = np.arange(n)
            out['matches that run into the last byte'] = int(((ln == n - p) & (ln >= 3)).sum())
            out['nice clipped by the lookahead, another candidate behind'] = int(
                ((tr['end'] == END_NICE) & (ln < CFG[level][3]) & (tr['beyond_len'] >= ln) & (ln >= 3)).sum())
        return out
    return Case('tail_%d' % n, tail_case.__doc__, data, cert)


def tail_mixed():
    """700 bytes of an 11-byte period: the last 64-slot group of the sorted order has lanes within 258 of the end and lanes
    further from it, so one wave takes both the clipped and the unclipped compare."""
    r = np.random.RandomState(77)
    data = (r.randint(0, 256, size=11).astype(np.uint8).tobytes() * 70)[:700]

    def cert(level, tr):
        s = sorted_window(data, tiles_of(700)[0])
        last = s[(len(s) - 1) // 64 * 64:]
        return {'last group: lanes within 258 of the end': int((700 - last < 258).sum()),
                'last group: lanes further away': int((700 - last >= 258).sum())}
    return Case('tail_mixed', tail_mixed.__doc__, data, cert)


# ---- tile seam ---------------------------------------------------------------------------------------------------------
SEAM_K = (-2, -1, 0, 1, 2, 3, 4, 64, 300, 40000)


def seam_case(k):
    """n = TILE + k random bytes with, where they fit: a 270-byte copy that begins 250 bytes before the seam (a 258-byte match
    across it, or one that runs into the end); positions just behind the seam whose only candidate lies in the halo at MAX_DIST
    (and one at MAX_DIST + 1); for k = 40000 the budget run of `budget` with every source before and every target behind the seam."""
    n = TILE + k
    pl = Plan(n, 900 + k % 997)
    owned, marks = {}, {}
    if k == 40000:
        m, T, pos = plant_budget_run(pl, TILE + 4)
        owned[hash3(*T)] = pos
        marks['budget'] = m
        marks['hash'] = hash3(*T)
    else:
        src = pl.rand(270)
        copy_at = TILE - 250
        pl.put(copy_at - 6000, b'\x10' + src + b'\x11')
        ln = min(270, n - copy_at)
        pl.put(copy_at, src[:ln])
        marks['copy'] = (copy_at, ln)
    if 64 <= k < 40000:
        for j, dd in ((24, MAX_DIST), (40, MAX_DIST + 1)):
            T = pl.rand(3); body = pl.rand(9)
            pl.put(TILE + j - dd, T + body + b'\x14'); pl.put(TILE + j, T + body + b'\x15')
            owned[hash3(*T)] = [TILE + j - dd, TILE + j]
            marks[dd] = TILE + j
    pl.scrub(owned)
    data = pl.bytes()

    def cert(level, tr):
        tl = tiles_of(n)
        out = {'tiles': len(tl)}
        a, ln = marks.get('copy', (0, 0))
        if k >= 1:
            out['the second tile owns positions'] = tl[1][3] - tl[1][0]
        if 1 <= k < 40000:
            out['a match begins before the seam and ends at or behind it'] = int(
                a < TILE and _len(tr['t_full'][a]) == min(258, ln) and a + min(258, ln) >= min(TILE + 1, n))
        if k <= 0:
            out['the first tile ends with the stream, a match runs into it'] = int(_len(tr['t_full'][n - 50]) == 50)
        if k >= 64 and k != 40000:
            p = marks[MAX_DIST]
            out['owned position behind the seam, winner in the halo at MAX_DIST'] = int(
                p >= TILE and tr['t_full'][p] == (12 << 16 | MAX_DIST) and p - MAX_DIST >= tl[1][1])
            out['and dropped at MAX_DIST + 1'] = int(tr['t_full'][marks[MAX_DIST + 1]] == 0 and tr['head_dist'][marks[MAX_DIST + 1]] == MAX_DIST + 1)
        if k == 40000:
            out.update(budget_cert(marks['budget'])(level, tr))
            c = CFG[level][0]
            out['the budget count straddles the seam'] = int(marks['budget'][c] >= TILE > marks['budget'][c] - 6 * c)
            # the run in the geometry of full-size tiles: 8 groups per k_match5 wave, 64 per k_match6 workgroup in the first tile
            for t, tile in enumerate(tl):
                a, e = run_slots(data, tile, marks['hash'])
                unit = 64 * (m5_groups_per_wave(tile[2]) if c <= 128 else m6_groups_per_workgroup(tile[2]))
                B = (e - 1) // unit * unit
                out['tile %d: the run lies on both sides of a %s start' % (t, 'wave' if c <= 128 else 'workgroup')] = int(a < B < e)
                if c > M6_WG_THREADS and t == 0:
                    B = (a + M6_WG_THREADS) // unit * unit + (unit if (a + M6_WG_THREADS) % unit else 0)
                    out['tile 0: more than 512 slots of it before a workgroup start (second look-back round)'] = int(B < e and B - a > M6_WG_THREADS)
        return out
    return Case('seam_%+d' % k, seam_case.__doc__, data, cert, marks=marks)


# ---- chunks back to back ---------------------------------------------------------------------------------------------
CHUNK_CUTS = (0, 7001, 19346, 19349, 31000, 40000)


def chunked_stream():
    """40000 bytes of a 5003-byte period, cut at CHUNK_CUTS (one chunk of 3 bytes among them): in the uncut stream every match
    reaches back over a cut and most go on over the next one; a chunk's matches must do neither."""
    r = np.random.RandomState(88)
    return (r.randint(0, 256, size=5003).astype(np.uint8).tobytes() * 8)[:CHUNK_CUTS[-1]]


# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in a fixed order."""
    cs = [budget()] + [run_case(N) for N in RUN_LENGTHS] + [collisions(), cmp_len(), nice(), dist_limits()]
    cs += [parse_case(lv) for lv in ALL]
    cs += [tail_case(n) for n in (3, 4, 5) + tuple(range(257, 265))] + [tail_mixed()]
    cs += [seam_case(k) for k in SEAM_K]
    return {c.name: c for c in cs}


def pairs():
    return [(name, lv) for name, c in cases().items() for lv in c.levels]


@functools.lru_cache(maxsize=None)
def zbytes(name, level):
    return zlib.compress(cases()[name].data, level)


@functools.lru_cache(maxsize=4)
def trace(name, level):
    from oracle import oracle as O
    return O.match_trace(cases()[name].data, level)


def explain(name, level, p):
    """What a failure report says about position p: where the kernel has it and how the reference walk went there."""
    from oracle import oracle as O
    tr = trace(name, level)
    return '%s level %d, position %d: %s; oracle walk: %d candidates, ended by %s, full winner is candidate %d, quarter winner %d, head at %d' % (
        name, level, p, locate(cases()[name].data, p), tr['visited'][p], O.END_NAMES[tr['end'][p]], tr['full_idx'][p], tr['quarter_idx'][p],
        tr['head_dist'][p])
