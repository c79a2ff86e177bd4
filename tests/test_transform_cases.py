"""CPU twin of tests/test_gpu_transform_edges.py: the cases of tests/transform_cases.py without a device.  The two references (the
reference's statement sequence on numpy, and the C oracle) must agree on every case, so that they pin each other; the ff_stream family
must give a stream of nothing but 0xff; the transition table must be what the restated rows_tile gives; and the case list must reach
every path of the row-tile kernels -- asserted with the restated predicates, a missing combination fails."""
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from tests import transform_cases as T

ROOT = Path(__file__).resolve().parent.parent


def test_transform_hip_names_this_file():
    src = (ROOT / 'mtscomp_amd' / 'csrc' / 'transform.hip').read_text()
    assert 'tests/transform_cases.py' in src
    assert 'ROWS_SCAN_PARTS = %d' % T.ROWS_SCAN_PARTS in src


@pytest.mark.parametrize('itemsize', [1, 2, 4])
def test_transition_table(itemsize):
    top = T.LDS_EDGE[itemsize][1] + 300
    tiles = [T.rows_tile(w, itemsize) for w in range(2, top)]
    assert all(a >= b for a, b in zip(tiles, tiles[1:]))                      # wider never means taller
    last = tuple(max(w for w, t in zip(range(2, top), tiles) if t == h) for h in (64, 32, 16))
    assert last == T.TRANSITIONS[itemsize]
    assert T.rows_tile(last[2] + 1, itemsize) == T.GENERIC and T.rows_tile(1, itemsize) == T.GENERIC
    # no width launches k_delta_rows with more LDS than the launcher asks for, static bytes included
    assert max(T.delta_rows_lds(w, itemsize) for w in range(2, top)) <= T.ROWS_LDS_LIMIT
    # the LDS-edge widths: a 17-row image within 64 KiB that the static bytes push over it
    edge = [w for w in range(2, top) if 17 * T.rows_pitch(w, itemsize) * itemsize <= T.ROWS_LDS_LIMIT
            < 17 * T.rows_pitch(w, itemsize) * itemsize + T.ROWS_STATIC_LDS]
    assert (edge[0], edge[-1]) == T.LDS_EDGE[itemsize] and edge == list(range(edge[0], edge[-1] + 1))
    assert all(17 * T.rows_pitch(w, itemsize) * itemsize + T.ROWS_STATIC_LDS == 65548 for w in edge)
    assert all(T.rows_tile(w, itemsize) == T.GENERIC for w in edge)
    # the case list sits on both sides of every transition, and on the edge
    ws = T.widths(itemsize)
    assert all(w in ws and w + 1 in ws for w in last) and set(T.LDS_EDGE[itemsize]) <= set(ws)
    assert {2, 3, 63, 64, 65, 385} <= set(ws)


def test_lds_edge_is_14_widths():
    assert sum(b - a + 1 for a, b in T.LDS_EDGE.values()) == 14
    assert T.widths(8) == [1, 2, 63, 64, 65, 129] and all(T.rows_tile(w, 8) == T.GENERIC for w in T.widths(8))


@pytest.mark.parametrize('dtype', [d for s in (1, 2, 4, 8) for d in T.DTYPES[s]])
def test_ff_stream_is_all_ff(dtype):
    for nt, nc in ((1, 1), (2, 3), (65, 7), (300, 2), (70000, 1)):                # (70000 rows: -(t + 1) wraps in 1- and 2-byte items)
        x = T.make('ff_stream', dtype, nt, nc)
        assert x.dtype == np.dtype(dtype) and x.shape == (nt, nc)
        s = T.np_stream(x)
        assert s.size == x.nbytes and np.all(s == 0xff)
        assert np.array_equal(O.delta_transpose(x, T.FLAGS_ROWS), s)


@pytest.mark.parametrize('dtype', [d for s in (1, 2, 4, 8) for d in T.DTYPES[s]])
def test_extremes_wrap_everywhere(dtype):
    x = T.make('extremes', dtype, 64, 9)
    info = np.iinfo(dtype)
    assert x.min() == info.min and x.max() == info.max
    d = T.np_stream(x).view(x.dtype).reshape(9, 64)[:, 1:]                        # the deltas of rows 1.., per channel
    moving = [c for c in range(9) if c not in (0, 4, 8)]
    want = {-1, 1} if info.min < 0 else {1, info.max}                             # max - min and min - max in the item's width
    assert set(np.unique(d[moving]).tolist()) == want
    assert not d[[0, 4, 8]].any()
    if x.dtype.itemsize == 4:                                                     # a tile's sums pass 2^32
        assert int(d[1].view(np.uint32).astype(np.uint64).sum()) > 1 << 32


@pytest.mark.parametrize('itemsize', [1, 2, 4, 8])
def test_numpy_reference_and_c_oracle_agree(itemsize):
    """Every single-chunk case, every all-flags case of the generic kernels and every chunk of every batch -- the lists the GPU tests
    run: the two references give the same stream, and both invert it."""
    cases = T.all_flags_cases(itemsize)
    n_flags = len(cases)
    # (3 widths, or the 6 of 8-byte items) x 12 row counts x 3 families x 2 dtypes x 8 flag sets
    assert n_flags == (6 if itemsize == 8 else 3) * 12 * 3 * 2 * 8
    assert {c[4] for c in cases} == set(range(8)) and {c[0] for c in cases} == set(T.WIDTHS_8 if itemsize == 8 else T.ALL_FLAGS_WIDTHS)
    for height in T.HEIGHTS:
        if not T.widths_of(itemsize, height):
            continue
        cases += [(w, nt, fam, dt, T.FLAGS_ROWS) for w, nt, fam, dt in T.single_cases(itemsize, height)]
        for w, rows, fam, dt in T.batch_cases(itemsize, height):
            cases += [(w, len(c), c, dt, T.FLAGS_ROWS) for c in T.batch_data(w, rows, fam, dt)[1]]
    for w, nt, fam, dt, fl in cases:
        x = fam if isinstance(fam, np.ndarray) else T.make(fam, dt, nt, w)
        s = T.np_stream(x, fl)
        assert np.array_equal(O.delta_transpose(x, fl), s), (w, nt, dt, fl)
        back = T.np_unstream(s, nt, w, dt, fl)
        assert back.dtype == x.dtype and back.flags.c_contiguous and np.array_equal(back, x), (w, nt, dt, fl)
        assert np.array_equal(O.cumsum_transpose(s, nt, w, dt, fl), x), (w, nt, dt, fl)
    # on top of the all-flags cases: every width of the cell at 12 row counts, 3 families and 2 dtypes, and the batches' chunks
    assert len(cases) >= n_flags + len(T.widths(itemsize)) * 12 * 3 * 2


@pytest.mark.parametrize('itemsize', [1, 2, 4])
def test_every_path_is_reached(itemsize):
    """Coverage as a condition: with the restated predicates, the case list reaches every tile height; per height both values of the
    stream-side predicate for K1 and for K2 (a whole tile next to a ragged one in one chunk among them); every store path an aligned
    item can take and both load paths, through the batches and the base offsets; k_rows_scan with 1, 7, 8, 9, 10 and 17 tiles; a
    batch with a chunk of fewer tiles than the longest."""
    assert {T.rows_tile(w, itemsize) for w in T.widths(itemsize)} == set(T.HEIGHTS)
    # (a 4-byte item at a multiple of 4 can never take the item-by-item stores: the rule mts_dev_decompress_chunks enforces)
    stores_wanted = {'vec16', 'dword', 'item'} if itemsize < 4 else {'vec16', 'dword'}
    ntiles = set()
    for tt in (64, 32, 16):
        ws = T.widths_of(itemsize, tt)
        assert ws and T.batch_widths(itemsize, tt) == [ws[0], ws[-1]]
        k1, k2, mixed = set(), set(), False
        for nt in T.row_counts(itemsize, tt):
            tiles = range(0, nt, tt)
            f1 = [T.stream_fast(tt, nt, t0, itemsize, False) for t0 in tiles]
            f2 = [T.stream_fast(tt, nt, t0, itemsize, True) for t0 in tiles]
            k1 |= set(f1)
            k2 |= set(f2)
            mixed |= len(set(f2)) == 2 and f1[-1] and not f2[-1]                 # whole tiles fast, the ragged last one not (K2), yet fast in K1
            ntiles.add(T.n_tiles(nt, tt))
        assert k1 == {True, False} and k2 == {True, False} and mixed, (tt, k1, k2, mixed)
        loads = set()                     # (per height: a row of 252 4-byte items is 63 * 16 bytes, every chunk of it starts aligned)
        for w in T.batch_widths(itemsize, tt):
            stores, gapped, fewer = set(), set(), False
            for rows in T.batches(itemsize, tt):
                nts = [T.n_tiles(r, tt) for r in rows]
                fewer |= min(nts) < max(nts)
                loads |= {T.load_path(a) for a in T.chunk_starts(rows, w, itemsize)}
                for base in T.BASES(itemsize):
                    stores |= {T.store_path(a, itemsize) for a in T.chunk_starts(rows, w, itemsize, base)}
                    gapped |= {T.store_path(a, itemsize) for a in T.chunk_starts(rows, w, itemsize, base, T.GAPS(itemsize)[1])}
            assert stores == stores_wanted, (tt, w, stores)
            assert gapped == stores_wanted, (tt, w, gapped)                      # and with a gap between the chunks
            assert fewer, (tt, w)
        assert loads == {'vec16', 'item'}, (tt, loads)
    assert {1, 7, 8, 9, 10, 17} <= ntiles, ntiles
    # k_rows_scan's parts: one tile per part or less (empty trailing parts), exactly one, two with an empty tail, three with a short tail
    for ntile in (1, 7, 8, 9, 10, 17):
        parts = T.scan_parts(ntile)
        assert len(parts) == T.ROWS_SCAN_PARTS and parts[0][0] == 0 and max(e for _, e in parts) == ntile
        assert all(a[1] == b[0] or b[0] == b[1] == ntile for a, b in zip(parts, parts[1:]))
        assert sum(e - b for b, e in parts) == ntile
    assert sum(b == e for b, e in T.scan_parts(1)) == 7 and sum(b == e for b, e in T.scan_parts(7)) == 1
    assert all(e - b == 1 for b, e in T.scan_parts(8)) and sum(b == e for b, e in T.scan_parts(9)) == 3
    assert [e - b for b, e in T.scan_parts(17)] == [3, 3, 3, 3, 3, 2, 0, 0]
    # the generic kernels: the LDS-edge widths and the first width behind them, and MTS_K12_GENERIC on every other width
    assert set(T.LDS_EDGE[itemsize]) < set(T.widths_of(itemsize, T.GENERIC))
