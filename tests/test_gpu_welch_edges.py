"""k_welch on the MI355X where a uniform bound cannot see it: every result against welch_f64 over the oracle's decode within the
bound per bin (welch_bound_bins), float32 and float64, on inputs whose bins lie far below the segment's energy (tones, a chirp, a
random walk, large offsets), on single segments of one or two impulses at rows chosen from the plan (a thread's first and last
row, both rows of a packed pair, rows on both sides of a chunk boundary) under a boxcar and two tapers without symmetry, on more
than two blocks of segments over a full tile and a tile of one live column for each of the 22 (compute type, nperseg) instances,
on columns whose power sits in bin 0 or bin N / 2, and exactly on 32, 33 and 70 segments.  Each case first asserts, from the
reference alone, that the bound is below what it is meant to see.  The cases come from tests/welch_oracle.py, where
tests/test_welch_oracles.py tries them on the CPU."""
import numpy as np
import pytest

from mtscomp_amd import api
from tests import welch_oracle as W
from tests.test_gpu_welch import _file, tmp_cfg  # noqa: F401

pytestmark = pytest.mark.gpu

NPERSEG = [1 << lg for lg in range(4, 15)]
CDTS = (np.float32, np.float64)
PLANS = [(np.dtype(cdt).name, lg) for cdt in CDTS for lg in range(4, 15)]


def _run(r, dec, nperseg, call, cdt, channels=None):
    """One Reader.welch call (start, stop, noverlap, window, detrend) against welch_f64 within welch_bound_bins.  -> (largest error
    / bound, the reference's sums, the bound, both unscaled, and the result)."""
    start, stop, noverlap, window, detrend = call
    cols = list(range(dec.shape[1])) if channels is None else channels
    _, got = r.welch(nperseg, start, stop, channels=cols, noverlap=noverlap, window=window, detrend='constant' if detrend else False, dtype=cdt)
    taper = api.welch_window(window, nperseg)
    tot, _, n_seg, first = W.welch_f64(dec[:, cols], start, stop, nperseg, nperseg - noverlap, taper, detrend, cdt)
    bins = W.welch_bound_bins(tot, first, n_seg)
    k = W.psd_scale(nperseg, taper, 'density', r.sample_rate, n_seg)[:, None]
    return W.assert_welch_close(got, tot * k, bins * k), tot, bins, got / k


def _cases(nperseg, which):
    return [c for c in W.edge_cases(nperseg) if (c[0] == which if which != 'structured' else c[3] is not None)]


@pytest.mark.parametrize('nperseg', NPERSEG)
def test_structured_spectra(tmp_cfg, nperseg):
    worst = {}
    for name, x, calls, shares in _cases(nperseg, 'structured'):
        r, dec = _file(tmp_cfg, x, rate=1000., chunk_duration=(nperseg + 3) * 1.37 / 1000., do_time_diff=x.dtype.kind != 'f')
        for call in calls:
            for cdt in CDTS:
                ratio, tot, bins, _ = _run(r, dec, nperseg, call, cdt)
                want = shares[call[4]] if cdt is np.float32 else (W.SHARE_F64,) * x.shape[1]
                share = (bins < tot).mean(axis=0)
                assert np.all(share >= np.array(want)), (name, call[4], cdt, share)      # (the bound is below the power it guards)
                key = np.dtype(cdt).name
                worst[key] = max(worst.get(key, 0.0), ratio)
        r.close()
    print('structured, nperseg %d: largest error / per-bin bound %s' % (nperseg, worst))


@pytest.mark.parametrize('nperseg', NPERSEG)
def test_sparse_segments(tmp_cfg, nperseg):
    """|X_k|^2 = (a0 w0)^2 + (a1 w1)^2 + 2 a0 w0 a1 w1 cos(2 pi k (n0 - n1) / N): both rows' positions and taper entries, every bin."""
    (_, x, calls, _), = _cases(nperseg, 'sparse')
    _, chunk_rows, starts, patterns = W.sparse_case(nperseg)
    r, dec = _file(tmp_cfg, x, rate=1000., chunk_duration=chunk_rows / 1000.)
    assert list(r.chunk_bounds[1:4]) == [chunk_rows * i for i in (1, 2, 3)]
    assert all(s0 < chunk_rows * (i + 1) <= s0 + nperseg for i, s0 in enumerate(starts))      # a chunk boundary inside each segment
    worst = {}
    for call in calls:
        w = api.welch_window(call[3], nperseg)
        for cdt in CDTS:
            ratio, tot, bins, _ = _run(r, dec, nperseg, call, cdt)
            assert np.all(bins < tot), (call[0], cdt)                            # every bin of every pattern holds more than the bound
            for j in (0, len(patterns) - 1):                                     # the reference is the closed form
                a = [float(x[call[0] + n, j]) * w[n] for n in patterns[j]]
                k = np.arange(nperseg // 2 + 1)
                want = a[0] ** 2 if len(a) == 1 else a[0] ** 2 + a[1] ** 2 + 2 * a[0] * a[1] * np.cos(2 * np.pi * k * (patterns[j][0] - patterns[j][1]) / nperseg)
                assert np.allclose(tot[:, j], want, rtol=1e-9, atol=1e-9 * (a[0] ** 2))
            key = np.dtype(cdt).name
            worst[key] = max(worst.get(key, 0.0), ratio)
    r.close()
    print('sparse, nperseg %d: largest error / per-bin bound %s' % (nperseg, worst))


@pytest.mark.parametrize('cdt_name,lg', PLANS, ids=['%s-%d' % (n, 1 << lg) for n, lg in PLANS])
def test_blocks_and_tiles(tmp_cfg, cdt_name, lg):
    """One k_welch instance: 70 segments (two full blocks of 32 and one of 6) on C + 1 columns (a full tile, and a tile whose other
    columns are dead), each segment with an amplitude of its own."""
    cdt, nperseg = np.dtype(cdt_name).type, 1 << lg
    x, channels = W.block_case(cdt, nperseg)
    C = W.welch_plan(cdt, nperseg)['C']
    n_seg = x.shape[0] // nperseg
    assert len(channels) == C + 1 and len(set(channels)) == C and n_seg > 2 * W.B and n_seg % W.B
    r, dec = _file(tmp_cfg, x, rate=30000., chunk_duration=max(x.shape[0] / 7.3, 100) / 30000.)
    ratio, tot, bins, _ = _run(r, dec, nperseg, (0, x.shape[0], 0, 'boxcar', False), cdt, channels)
    r.close()
    # a segment missing or added twice moves every bin by its power, amplitude^2 >= 1000^2: more than the bound
    seg_power = np.abs(dec.astype(np.float64)).reshape(n_seg, nperseg, C).max(axis=1) ** 2          # (n_seg, C): a boxcar, every bin
    assert seg_power.min() >= 1e6 and seg_power.min() > bins.max(), (seg_power.min(), bins.max())
    print('blocks %s %d (C = %d): largest error / per-bin bound %.3g, bound / smallest segment power %.3g'
          % (cdt_name, nperseg, C, ratio, bins.max() / seg_power.min()))


@pytest.mark.parametrize('nperseg', NPERSEG)
def test_bin_0_and_bin_half(tmp_cfg, nperseg):
    """Bins 0 and N / 2 come from Z[0] alone (acc_m, k == 0).  Boxcar: a (-1)^n gives (N a)^2 in bin N / 2 and 0 elsewhere, a constant
    v gives (N v)^2 in bin 0, exactly.  Hann: the neighbours (N / 2 - 1, 1) get a quarter of it and the rest next to nothing."""
    N = nperseg
    (_, x, calls, _), = _cases(nperseg, 'one_bin')
    r, dec = _file(tmp_cfg, x, rate=1000., chunk_duration=max(N, 300) * 0.41 / 1000.)
    n_seg = 4
    for cdt in CDTS:
        _, p = r.welch(N, 0, n_seg * N, noverlap=0, window='boxcar', detrend=False, scaling='spectrum', dtype=cdt)
        k = np.full(N // 2 + 1, 2.0 / float(N) ** 2)                    # powers of two and n_seg = 4: undone exactly, as in test_exact_cases
        k[0] = k[-1] = 1.0 / float(N) ** 2
        want = np.zeros((N // 2 + 1, 3))
        want[-1, 0] = n_seg * float(N * 1500) ** 2
        want[0, 1] = n_seg * float(N * 1234) ** 2
        want[-1, 2], want[0, 2] = n_seg * float(N * 77) ** 2, n_seg * float(N * 5) ** 2
        assert want.max() < 2.0 ** 53
        assert np.array_equal(p, want * k[:, None] / n_seg), cdt
        for call in calls:
            ratio, tot, bins, got = _run(r, dec, N, call, cdt)
            rest = np.ones(N // 2 + 1, bool)
            rest[[0, 1, N // 2 - 1, N // 2]] = False
            if N >= 8 and rest.any():
                # from the reference: the leakage bin holds a quarter of the main one and is far above its bound, the rest is rounding
                assert abs(tot[N // 2 - 1, 0] / tot[N // 2, 0] - 0.25) < 1e-9 and bins[N // 2 - 1, 0] < 1e-3 * tot[N // 2 - 1, 0]
                assert tot[rest].max() < 1e-20 * tot.max()
                assert abs(got[N // 2 - 1, 0] / got[N // 2, 0] - 0.25) < 1e-3
                assert got[rest][:, 0].max() <= bins[rest][:, 0].max() < 1e-8 * tot[N // 2, 0]
                if not call[4]:
                    assert abs(got[1, 1] / got[0, 1] - 0.25) < 1e-3 and got[rest][:, 1].max() < 1e-8 * tot[0, 1]
            print('one bin, nperseg %d %s detrend %s: largest error / per-bin bound %.3g' % (N, np.dtype(cdt).name, call[4], ratio))
    r.close()


@pytest.mark.parametrize('n_seg', [32, 33, 70])
def test_exact_cases_full_blocks(tmp_cfg, n_seg):
    """test_exact_cases' impulse and piecewise-constant columns on a full block, a block and one segment, and two blocks and a part.
    Why exact: an impulse a at a segment's row 0 is the real part of point 0, which no pass multiplies by a twiddle (slot r = 0),
    so every bin is a in either compute type; a constant v makes every point v + i v, whose sums N v / 2 <= 2^13 * 35 < 2^24 are
    integers that float32 holds and whose differences are 0.  Every term is an integer: a <= 212 gives a^2 < 2^16, |v| <= 35 gives
    (N v)^2 <= (2^14 * 35)^2 < 2^39, so the sums of 70 stay far below 2^53 and the float64 additions are exact in any order."""
    nc = 3
    for nperseg in (16, 256, 1024, 16384):
        rows = nperseg * n_seg + 3
        x = np.zeros((rows, nc), np.int16)
        a = np.arange(1, n_seg + 1) * 3 + 2
        x[np.arange(n_seg) * nperseg, 0] = a                              # impulses at row 0: point 0's real part, no twiddle but 1
        v = np.arange(n_seg) - 34
        x[:nperseg * n_seg, 1] = np.repeat(v, nperseg)
        x[nperseg * n_seg:, 1] = 1000
        x[:, 2] = -123
        r, _ = _file(tmp_cfg, x, rate=1000., chunk_duration=max(nperseg, 700) * 0.37 / 1000.)
        for cdt in CDTS:
            _, p = r.welch(nperseg, 0, nperseg * n_seg, noverlap=0, window='boxcar', detrend=False, scaling='spectrum', dtype=cdt)
            k = np.full(nperseg // 2 + 1, 2.0 / float(nperseg) ** 2)
            k[0] = k[-1] = 1.0 / float(nperseg) ** 2
            want0 = np.zeros(nperseg // 2 + 1) + float(sum(int(q) ** 2 for q in a))
            want1 = np.zeros(nperseg // 2 + 1)
            want1[0] = float(sum((nperseg * int(q)) ** 2 for q in v))
            assert want0[0] < 2.0 ** 53 and want1[0] < 2.0 ** 53
            # the reference divides as Reader.welch does: the exact sum times the bin's scale, divided by n_seg
            assert np.array_equal(p[:, 0], want0 * k / n_seg), (nperseg, cdt)
            assert np.array_equal(p[:, 1], want1 * k / n_seg), (nperseg, cdt)
            _, p = r.welch(nperseg, 0, nperseg * n_seg, noverlap=0, window='hann', detrend='constant', dtype=cdt)
            assert not p[:, [1, 2]].any(), (nperseg, cdt)
        r.close()
