"""The exact references of the reduction kernels, on the CPU: the integer FIR of tests/decimate_oracle.py against the numpy
restatement of k_decimate, the launch-plan copy and the case matrix the GPU tests take from it, and the fsum bound of
tests/stats_oracle.py against the numpy restatement of mts_window_stats.  A reference that is wrong here cannot be trusted on the
device (tests/test_gpu_reduce_edges.py)."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api
from tests.decimate_oracle import (DECIMATE_PLAN_CASES, PLAN_BRANCHES, dec_plan, dyadic_taps, exact_tap_budget, fir_decimate,
                                   fir_decimate_exact, plan_branches, plan_n_outs)
from tests.stats_oracle import (StatsOracleCodec, assert_stats_exact_bound, gamma, stat_tiles_per_window, stats_depth)


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


# ---- decimation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out_dtype', ['float32', 'float64'])
@pytest.mark.parametrize('q,n_taps', [(1, 1), (2, 5), (3, 64), (12, 241), (7, 1000), (300, 8192)])
def test_exact_fir_equals_the_restatement_on_representable_inputs(out_dtype, q, n_taps):
    rs = np.random.RandomState(q * 7919 + n_taps)
    n_out = 9
    rows = n_taps + (n_out - 1) * q + 40
    x = rs.randint(-2047, 2048, size=(rows, 3)).astype(np.int16)
    x[rs.randint(0, rows, 5), 0] = 2047                       # (the extremes of the range are there)
    k, s, taps = dyadic_taps(rs, n_taps, exact_tap_budget(2047, out_dtype))
    for vb, ve in ((0, rows), (n_taps // 2, rows - 7), (5, 5)):
        first = n_taps - 1 + 3
        want = fir_decimate_exact(x, 0, vb, ve, first, n_out, q, k, s, out_dtype)
        got = fir_decimate(x, 0, vb, ve, first, n_out, q, taps, out_dtype)
        assert want.dtype == np.dtype(out_dtype) and got.tobytes() == want.tobytes()
        # it is not the restatement's twin: a dropped last tap, a row off by one, the taps reversed all differ from it
        bad = [fir_decimate(x, 0, vb, ve, first, n_out, q, taps[:-1], out_dtype) if n_taps > 1 else None,
               fir_decimate(x, 0, vb, ve, first + 1, n_out, q, taps, out_dtype),
               fir_decimate(x, 0, vb, ve, first, n_out, q, taps[::-1], out_dtype) if n_taps > 1 and not np.array_equal(taps, taps[::-1]) else None]
        if vb == 0:                                           # (with vb > 0 the last tap may only read zeros)
            for b in bad:
                assert b is None or b.tobytes() != want.tobytes()


def test_exact_fir_refuses_what_it_cannot_represent():
    x = np.full((20, 1), 2 ** 12, np.int32)
    k = np.full(4, 1 << 11, np.int64)                         # sum |k| * max|x| = 2^25 > 2^24
    with pytest.raises(AssertionError, match='not exactly representable'):
        fir_decimate_exact(x, 0, 0, 20, 5, 3, 2, k, 0, 'float32')
    fir_decimate_exact(x, 0, 0, 20, 5, 3, 2, k, 0, 'float64')
    with pytest.raises(AssertionError, match='not integers'):
        fir_decimate_exact(x + 0.5, 0, 0, 20, 5, 3, 2, k[:1], 0, 'float64')


def test_dyadic_taps_keep_the_budget_and_both_ends():
    rs = np.random.RandomState(0)
    for n_taps in (1, 2, 3, 255, 8192):
        for budget in (1, 2, 8192, 1 << 40):
            if budget < min(n_taps, 2):
                continue
            k, s, t = dyadic_taps(rs, n_taps, budget)
            assert k.size == n_taps and np.abs(k).sum() <= budget and k[0] != 0 and k[-1] != 0
            assert np.array_equal(t * 2.0 ** s, k.astype(np.float64))


def test_dec_plan_copy_matches_the_kernel_formula():
    # hand-worked from decimate.hip's dec_plan<F>: S = 65536 / (64 * sizeof(F)), to = min((S - min(L, 32)) / q + 1, 64), ...
    assert dec_plan(241, 12, 'float32') == (256, 2, 16, 64)           # to = 224 / 12 + 1 = 19
    assert dec_plan(3, 40, 'float32') == (256, 1, 7, 16)              # to = 253 / 40 + 1 = 7, slab = 256 - 6 * 40
    assert dec_plan(2, 2, 'float64') == (128, 8, 64, 2)               # to = 126 / 2 + 1 = 64, slab = 128 - 63 * 2
    assert dec_plan(3, 2, 'float64') == (128, 4, 32, 64)                # to = 63: R = 4, slab = min(66, 64)
    assert dec_plan(8192, 256, 'float32') == (256, 1, 1, 64)
    for q in range(1, 600):
        for n_taps in (1, 2, 31, 32, 33, 200, 8192):
            for f in ('float32', 'float64'):
                S, R, to, slab = dec_plan(n_taps, q, f)
                assert 1 <= to <= 8 * R and 1 <= min(n_taps, 32) <= slab <= 64
                assert (to - 1) * q + slab <= S                    # the tile's rows and one slab fit the ring


def test_plan_case_matrix_covers_every_branch():
    reached = set()
    for q, n_taps, f in DECIMATE_PLAN_CASES:
        for n_out in plan_n_outs(n_taps, q, f):
            reached |= plan_branches(n_taps, q, f, n_out)
    assert reached >= PLAN_BRANCHES, sorted(PLAN_BRANCHES - reached)
    print('dec_plan branches reached:', ' '.join(sorted(reached)))


# ---- window statistics ---------------------------------------------------------------------------------------------------------
def test_stat_tiling_restatement():
    b = [0, 1, 513, 1100, 1101, 3000]
    tiles, big = stat_tiles_per_window(b, 0, 3000, 1000)
    # window 0: [0, 1) [1, 513) [513, 1000): 1 + 1 + 1; window 1: [1000, 1100) [1100, 1101) [1101, 2000): 1 + 1 + 2; window 2: 2
    assert tiles.tolist() == [3, 4, 2] and big.tolist() == [512, 512, 512]
    tiles, big = stat_tiles_per_window(b, 5, 40, 7)
    assert tiles.tolist() == [1] * 5 and big.tolist() == [7] * 5
    assert stats_depth(b, 5, 40, 7).tolist() == [2 + 4 + 1 + 1 + 1] * 5
    assert float(gamma(1)) == pytest.approx(2.0 ** -53)


@pytest.mark.parametrize('dtype', ['float32', 'float64', 'int32', 'uint32', 'int64', 'uint64', 'int16', 'uint8'])
@pytest.mark.parametrize('n_lanes', [1, 2])
def test_exact_bound_holds_for_the_numpy_restatement(tmp_cfg, dtype, n_lanes):
    rs = np.random.RandomState(5)
    dt = np.dtype(dtype)
    rows, nc = 3000, 4
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 10. ** rs.randint(-5, 6, size=(1, nc))).astype(dt)
        x[17, 1] = np.nan
        x[900:1000, 2] = np.inf
        x[100:300, 3] = np.finfo(dt).tiny / 8                    # subnormals
        if dt == np.float64:
            x[2500:2600, 0] = 1e200                               # (x^2 overflows)
    else:
        info = np.iinfo(dt)
        x = rs.randint(info.min, int(info.max) + 1, size=(rows, nc), dtype=dt if dt.itemsize == 8 else np.int64).astype(dt)
        x[:, 0] = info.max
        x[::2, 1] = info.min
    codec = StatsOracleCodec(n_lanes=n_lanes, capacity_chunks=8)
    raw = tmp_cfg / 'data.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', sample_rate=1000., n_channels=nc, dtype=dt, codec=codec,
                         do_time_diff=dt.kind != 'f', check_after_compress=False)
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    dec = r[:]
    for window, start, stop in ((1000, 0, rows), (513, 11, 2990), (1, 995, 1010), (None, 0, rows)):
        got = r.window_stats(window, start, stop)
        w = window or stop - start
        assert assert_stats_exact_bound(got, dec, r.chunk_bounds, start, stop, w, range(nc), parts=n_lanes) == got['sum'].size
    # and the bound sees one tile too many or too few: a float sum off by one tile's partial, an integer sum off by one item
    got = r.window_stats(1000, 0, rows, channels=[0])
    wrong = dict(sum=got['sum'].copy(), sumsq=got['sumsq'].copy())
    if dt.kind == 'f':
        wrong['sum'][1, 0] += dec[1000:1512, 0].astype(np.float64).sum()          # (column 0 is finite in rows 1000..2000)
    else:
        wrong['sum'][1, 0] = np.int64(wrong['sum'][1, 0]) ^ np.int64(1)
    with pytest.raises(AssertionError):
        assert_stats_exact_bound(wrong, dec, r.chunk_bounds, 0, rows, 1000, [0], parts=n_lanes)
    r.close()
