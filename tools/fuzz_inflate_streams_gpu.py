"""Randomised inflate parity on streams no encoder writes, on a GPU box: random token sequences cut into random blocks of all
three types, dynamic blocks with length-limited trees of a random depth over perturbed counts (tests/deflate_build.py), 64
streams a round, a third of them made invalid by one structural edit (a distance past the first byte, a forbidden symbol, a
broken code length, a cut).  zlib gives the verdict for each stream on the CPU; all 64 go through ONE decompress_chunks call,
and every status and every byte must be zlib's.  A mismatch prints the seed and the stream's index and leaves the stream in
the temporary directory.

    python tools/fuzz_inflate_streams_gpu.py [seed] [seconds]
"""
import os
import sys
import tempfile
import time
import zlib
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from mtscomp_amd import hip  # noqa: E402
from tests import deflate_build as D  # noqa: E402

STREAMS = 64
EDITS = ('distance', 'symbol', 'length', 'cut')


def tokens_of(r):
    """A token sequence of up to 20 KB of output over a small alphabet (so that copies exist), and its bytes."""
    target = int(r.choice([1, 3, 40, 600, 5000, 20000]) * r.uniform(0.3, 1.0)) + 1
    k = int(r.choice([1, 2, 4, 16, 64]))
    p_copy = float(r.choice([0.0, 0.1, 0.5, 0.9]))
    toks, nout = [], 0
    while nout < target:
        if nout and r.uniform() < p_copy:
            ln = int(r.choice([3, 4, 8, 9, 10, 11, 16, 17, 257, 258])) if r.randint(0, 2) else int(r.randint(3, 259))
            far = min(nout, 32768)
            d = (far, 1, int(r.randint(1, min(far, 9) + 1)), int(r.randint(1, far + 1)))[int(r.randint(0, 4))]
            toks.append((258, d, 284) if ln == 258 and r.randint(0, 2) else (ln, d))
            nout += ln
        else:
            toks.append(int(r.randint(0, k)))
            nout += 1
    return toks


def sizes_of(toks):
    return [1 if isinstance(t, int) else t[0] for t in toks]


def build(r, toks, edit):
    """One stream from `toks`: 1 .. 12 blocks of random types.  edit: None or one of EDITS.  Returns the stream."""
    toks = list(toks)
    data = D.expand(toks)
    nb = int(r.randint(1, 13))
    cuts = sorted(int(x) for x in r.randint(0, len(toks) + 1, size=nb - 1))
    cuts = [0] + cuts + [len(toks)]
    types = [int(x) for x in r.randint(0, 3, size=nb)]
    off = np.concatenate(([0], np.cumsum(sizes_of(toks)))).astype(np.int64)
    victim = int(r.randint(0, nb))                         # the block an edit goes to
    if edit == 'distance':
        copies = [i for i, t in enumerate(toks) if not isinstance(t, int) and off[i] < 32768]
        if not copies:
            edit = 'symbol'
        else:
            i = copies[int(r.randint(0, len(copies)))]
            toks[i] = (toks[i][0], int(off[i]) + 1 + int(r.randint(0, 2)) * int(r.randint(0, 50)))
            if toks[i][1] > 32768:
                toks[i] = (toks[i][0], int(off[i]) + 1)
            for b in range(nb):                            # (a stored block has no copies)
                if cuts[b] <= i < cuts[b + 1] and types[b] == 0:
                    types[b] = 1 + int(r.randint(0, 2))
    w = D.Writer()
    for b in range(nb):
        part = toks[cuts[b]:cuts[b + 1]]
        final = b == nb - 1
        kind = types[b]
        if edit == 'symbol' and b == victim:
            kind = 1                                       # the fixed code has codes for the symbols no stream may use
            at = int(r.randint(0, len(part) + 1))
            bad = [('raw', 'l', int(r.choice([286, 287])), 0, 0)] if r.randint(0, 2) else \
                [('raw', 'l', int(r.randint(257, 265)), 0, 0), ('raw', 'd', int(r.choice([30, 31])), 0, 0)]
            part = part[:at] + bad + part[at:]
        if edit == 'length' and b == victim:
            kind = 2
        if kind == 0:
            w.stored(data[int(off[cuts[b]]):int(off[cuts[b + 1]])], final)
        elif kind == 1:
            w.fixed(part, final)
        else:
            maxbits = int(r.randint(7, 16))
            lf, df = D.token_counts(part)
            for f in (lf, df):                             # counts perturbed: not the trees zlib would build
                for s in range(len(f)):
                    if f[s]:
                        f[s] *= int(r.randint(1, 9))
                    elif r.uniform() < 0.05:
                        f[s] = int(r.randint(1, 4))
            if sum(1 for x in lf if x) > 1 << maxbits:
                maxbits = 9
            ll, dl = D.limited_lengths(lf, maxbits), D.limited_lengths(df, maxbits)
            if edit == 'length' and b == victim:
                lens = ll if r.randint(0, 3) else dl
                used = [s for s, l in enumerate(lens) if l]
                s = used[int(r.randint(0, len(used)))]
                lens[s] += 1 if lens[s] == 1 or (lens[s] < 15 and r.randint(0, 2)) else -1
            w.dynamic(part, final, lit_lens=ll, dist_lens=dl)
    z = D.zwrap(w, data)
    if edit == 'cut':
        z = z[:int(r.randint(0, len(z)))]
    return z


def verdict(z, n):
    try:
        out = zlib.decompress(z)
    except zlib.error:
        return hip.CHUNK_CORRUPT, None
    return (0, out) if len(out) == n else (hip.CHUNK_BADSIZE, None)


def one_round(r):
    streams, rows, want, edits = [], [], [], []
    for _ in range(STREAMS):
        toks = tokens_of(r)
        edit = EDITS[int(r.randint(0, len(EDITS)))] if r.randint(0, 3) == 0 else None
        z = build(r, toks, edit)
        n = sum(sizes_of(toks))
        streams.append(z)
        rows.append(n)
        want.append(verdict(z, n))
        edits.append(edit)
    st, arrs = hip.decompress_chunks(streams, rows, 1, 'uint8', 0)
    bad = []
    for i in range(STREAMS):
        if st[i] != want[i][0] or (st[i] == 0 and arrs[i].tobytes() != want[i][1]):
            bad.append((i, edits[i], want[i][0], st[i], streams[i]))
    return bad, sum(1 for w in want if w[0] != 0)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261020))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 5))
    print('fuzz_inflate_streams_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
    hip.require_device()
    t_end = time.time() + seconds
    rounds = refused = mism = 0
    while rounds == 0 or time.time() < t_end:
        bad, nref = one_round(np.random.RandomState([seed, rounds]))
        refused += nref
        for i, edit, want, got, z in bad:
            path = Path(tempfile.gettempdir()) / ('fuzz_inflate_streams_%d_%d_%d.z' % (seed, rounds, i))
            path.write_bytes(z)
            print('MISMATCH seed %d round %d stream %d (edit %s): zlib says %d, the device %d; stream of %d bytes in %s'
                  % (seed, rounds, i, edit, want, got, len(z), path), flush=True)
        mism += len(bad)
        rounds += 1
    print('fuzz_inflate_streams_gpu seed %d: %d rounds, %d streams, %d refused by zlib, %d mismatches' % (seed, rounds, rounds * STREAMS, refused, mism))
    return 1 if mism else 0


if __name__ == '__main__':
    sys.exit(main())
