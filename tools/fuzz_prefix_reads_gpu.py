"""Randomised safety of the leading-channel prefix decode, on a GPU box: a case draws a dtype, the transform flags, a row count, a
leading count k, who wrote the stream (zlib level 1 / 6 / 9, Z_FIXED, stored only, a sync or full flush near the end of the
prefix, tests/deflate_build.Writer with a stored or fixed block over it) and a handful of lengths L -- random ones, the ones
around L_min (the byte that ends the block that completes the prefix) and the ones around the end of the chunk.  Before every call
another chunk of the same shape is decoded whole through the same engine.  mts_cache_read_slices_leading with the first L bytes
must answer MTS_E_MISS, or status 0 and exactly arr[rows, :k]; with the whole chunk and no n_leading it must answer arr.  A
mismatch prints the seed and the case and leaves the stream in the temporary directory.

    python tools/fuzz_prefix_reads_gpu.py [seed] [cases]
"""
import os
import sys
import tempfile
import zlib
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from mtscomp_amd import hip  # noqa: E402
from tests import prefix_cases as P  # noqa: E402

WRITERS = ('zlib1', 'zlib6', 'zlib9', 'fixed', 'stored', 'sync', 'full', 'w_stored', 'w_fixed_short', 'w_fixed_long', 'w_exact')


def draw(r, index):
    dtype = np.dtype(str(r.choice(['uint8', 'int16', 'int16', 'int32', 'int64'])))
    flags = P.FLAGS[int(r.randint(0, 4))]
    nc = int(r.choice([130, 96, 33]))
    rows = int(r.choice([0, 1, 2, 63, 64, 300, 301, 700]))
    k = int(r.choice([1, 2, 3, 16, 63, 64, 65, nc - 1, int(r.randint(1, nc))]))
    k = min(k, nc - 1)
    writer = WRITERS[int(r.randint(0, len(WRITERS)))]
    arr = P.signal(dtype, rows, int(r.randint(0, 1 << 30)), nc=nc, const_lead=k if r.randint(0, 8) == 0 else 0)
    stream = P.stream_of(arr, flags)
    need = rows * k * dtype.itemsize
    if writer.startswith('zlib'):
        z = P.zlib_stream(stream, int(writer[4:]))
    elif writer == 'fixed':
        z = P.zlib_stream(stream, 6, zlib.Z_FIXED)
    elif writer == 'stored':
        z = P.zlib_stream(stream, 0)
    elif writer in ('sync', 'full'):
        cut = min(max(need + int(r.randint(-1, 2)), 0), len(stream))
        z = P.zlib_stream(stream, 6, cut=cut, flush=zlib.Z_SYNC_FLUSH if writer == 'sync' else zlib.Z_FULL_FLUSH)
    else:
        kind, size, before = {'w_stored': (0, 3000, 1000), 'w_fixed_short': (1, 2000, 1000), 'w_fixed_long': (1, 8000, 3000),
                              'w_exact': (2, 5000, 5000)}[writer]
        if len(stream) > 150000:                                  # (the Python writer: keep it short)
            arr = arr[:150000 // (nc * dtype.itemsize)]
            stream = P.stream_of(arr, flags)
            need = arr.shape[0] * k * dtype.itemsize
        z, _ = P.written(stream, P._plan_around(need, kind, size, min(before, need), max(len(stream), 1)) if stream else [(2, 0)])
    case = P.Case('fuzz_%d_%s_%s_f%d_%dx%d_k%d' % (index, writer, dtype.name, flags, arr.shape[0], nc, k), arr, flags, z, (k,), writer)
    n, lm = len(z), case.l_min(k)
    ls = {lm + d for d in range(-2, 3)} | {n - d for d in range(5)} | {int(x) for x in r.randint(2, n + 1, size=4)}
    return case, k, sorted(x for x in ls if 2 <= x <= n)


def run_case(cid, case, k, lengths, key):
    """-> list of (length, what went wrong)."""
    bad = []
    rows, nc = case.arr.shape
    other = zlib.compress(P.stream_of((case.arr[::-1] ^ 0x55).astype(case.dtype), P.FLAGS[0]), 1) if rows else None
    reqs = [(0, rows, 1, 0, k, 1), (min(1, rows), rows, 3, (k - 1) % 2, k, 2)]
    for length in lengths + [None]:
        if other is not None:
            st, _ = hip.decompress_chunks([other], [rows], nc, case.dtype, P.FLAGS[0])
            if st != [0]:
                bad.append((length, 'the poison chunk did not decode: %s' % st))
        key[0] += 1
        try:
            if length is None:                                    # the whole chunk, every channel, every check
                st, got = hip.cache_read_slices(cid, [key[0]], case.z, [0], [len(case.z)], [rows], nc, case.dtype, case.flags, [(0, rows, 1, 0, nc, 1)])
                if st != [0] or not np.array_equal(got[0], case.arr):
                    bad.append((length, 'whole decode: status %s' % st))
                continue
            st, got = hip.cache_read_slices(cid, [key[0]], case.z[:length], [0], [length], [rows], nc, case.dtype, case.flags, reqs, n_leading=k)
        except hip.HipError as e:
            if e.code != hip.E_MISS or length is None:
                bad.append((length, 'error %d: %s' % (e.code, e)))
            continue
        if st != [0]:
            bad.append((length, 'status %s' % st))
        elif not all(np.array_equal(g, case.arr[rb:re:rs, cb:ce:cs]) for g, (rb, re, rs, cb, ce, cs) in zip(got, reqs)):
            bad.append((length, 'wrong bytes'))
    return bad


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261021))
    count = int(sys.argv[2]) if len(sys.argv) > 2 else int(os.environ.get('MTS_FUZZ_CASES', 24))
    print('fuzz_prefix_reads_gpu: seed %d, %d cases' % (seed, count), flush=True)
    hip.require_device()
    cid = hip.cache_create(1 << 28)
    key, mism, calls, ok = [0], 0, 0, 0
    try:
        for index in range(count):
            case, k, lengths = draw(np.random.RandomState([seed, index]), index)
            bad = run_case(cid, case, k, lengths, key)
            calls += len(lengths) + 1
            for length, what in bad:
                path = Path(tempfile.gettempdir()) / ('%s_seed%d.z' % (case.name, seed))
                path.write_bytes(case.z)
                print('MISMATCH seed %d case %d (%s) L=%s of %d, L_min %d: %s; stream in %s' % (seed, index, case.name, length, len(case.z), case.l_min(k), what, path),
                      flush=True)
            mism += len(bad)
            ok += not bad
    finally:
        hip.cache_destroy(cid)
    print('fuzz_prefix_reads_gpu seed %d: %d cases, %d calls, %d mismatches' % (seed, count, calls, mism))
    return 1 if mism else 0


if __name__ == '__main__':
    sys.exit(main())
