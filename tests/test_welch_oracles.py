"""The references the Welch kernel is held to, tested on the CPU: the plan restated in welch_oracle against welch.hip, a numpy
restatement of the kernel's transform (kernel_rfft: the kernel's index arithmetic in the compute type) against numpy's FFT, that
honest implementation within the per-bin bound on every deterministic edge case, the per-bin bound never above the uniform one, and
five in-bounds mistakes put into the restatement: which of them the per-bin bound sees, and which the uniform bound would have
passed (printed; run with -s)."""
import re
from pathlib import Path

import numpy as np
import pytest

from mtscomp_amd import api, hip
from tests import welch_oracle as W

SRC = (Path(hip.__file__).resolve().parent / 'csrc' / 'welch.hip').read_text()
NPERSEG = [1 << lg for lg in range(4, 15)]
CDTS = (np.float32, np.float64)
EPS = np.finfo(np.float64).eps


def _ratio(got, tot, bound):
    """The largest |got - tot| / bound."""
    return float((np.abs(got - tot) / (bound + np.finfo(np.float64).tiny)).max())


def _ref(x, call, nperseg, cdt):
    start, stop, noverlap, window, detrend = call
    taper = api.welch_window(window, nperseg)
    tot, energy, n_seg, first = W.welch_f64(x, start, stop, nperseg, nperseg - noverlap, taper, detrend, cdt)
    return taper, tot, W.welch_bound_bins(tot, first, n_seg), W.welch_bound(nperseg, cdt, energy, n_seg)[None, :]


def test_plan_restatement_matches_the_kernel():
    header = (Path(hip.__file__).resolve().parent.parent / 'include' / 'mtscomp_hip.h').read_text()
    assert W.B == hip.WELCH_BLOCK_SEGMENTS == int(re.search(r'#define MTS_WELCH_BLOCK_SEGMENTS (\d+)', header).group(1))
    assert W.WT == int(re.search(r'constexpr int WT = (\d+);', SRC).group(1))
    assert W.TILE_BYTES == int(re.search(r'constexpr long WELCH_TILE_BYTES = (\d+);', SRC).group(1))
    assert 'C * N * sizeof(F) <= 64 KiB; 128 KiB for float64 at N = 16384' in SRC
    assert hip.WELCH_MAX_NPERSEG == NPERSEG[-1]
    for cdt in CDTS:
        size = np.dtype(cdt).itemsize
        for N in NPERSEG:
            p = W.welch_plan(cdt, N)
            assert p['C'] * p['P'] == W.WT and p['P'] * p['K'] == N and p['BINS'] * W.WT == (N // 2) * p['C']
            assert p['C'] & (p['C'] - 1) == 0 and 1 <= p['C'] <= 64 and p['K'] >= 2 and p['BINS'] >= 1
            # the header's LDS arithmetic: as many columns as 64 KiB hold, 64 at the most; one column of float64 at 16384 takes 128 KiB
            assert p['lds'] == p['C'] * N * size
            assert p['lds'] <= 65536 or (cdt is np.float64 and N == 16384 and p['C'] == 1 and p['lds'] == 131072)
            assert p['C'] == 64 or 2 * p['lds'] > 65536
            assert (p['C'] == 64) == (N <= (256 if cdt is np.float32 else 128))
    assert W.welch_plan(np.float32, 16384) == dict(C=1, P=512, K=32, BINS=16, lds=65536)
    assert W.welch_plan(np.float64, 16) == dict(C=64, P=8, K=2, BINS=1, lds=8192)


@pytest.mark.parametrize('nperseg', NPERSEG)
def test_kernel_rfft_matches_numpy(nperseg):
    """The index formulas of fft_pass and the split: every bin of the restated transform within delta_F sqrt(N E) of numpy's."""
    rs = np.random.RandomState(nperseg)
    y = rs.randn(nperseg, 5) * 1000
    y[:, 3] = 0
    y[nperseg // 2 + 1, 3] = 1.0                                         # an impulse at an odd row
    y[:, 4] = np.cos(2 * np.pi * 3 * np.arange(nperseg) / nperseg)      # bin 3 (the packed transform's and the split's symmetry)
    for cdt in CDTS:
        yf = y.astype(cdt)
        re, im = W.kernel_rfft(yf, cdt)
        assert re.dtype == im.dtype == np.dtype(cdt)
        X = np.fft.rfft(yf.astype(np.float64), axis=0)
        e = W.welch_delta(nperseg, cdt) * np.sqrt(nperseg * (yf.astype(np.float64) ** 2).sum(axis=0))
        assert np.all(np.abs((re.astype(np.float64) + 1j * im.astype(np.float64)) - X) <= e[None, :])
    X = np.fft.rfft(y[:, 3])
    re, im = W.kernel_rfft(y[:, 3:4], np.float64)
    assert np.abs(re[:, 0] + 1j * im[:, 0] - X).max() < 1e-14 and abs(np.abs(X) - 1).max() < 1e-14


@pytest.mark.parametrize('nperseg', NPERSEG)
def test_restatement_within_the_bin_bound_and_bin_bound_below_uniform(nperseg):
    worst = {}
    for name, x, calls, shares in W.edge_cases(nperseg):
        for call in calls:
            for cdt in CDTS:
                taper, tot, bins, uniform = _ref(x, call, nperseg, cdt)
                # equal where a bin holds all the energy, up to the rounding of the two expressions (a few ulps of float64)
                assert np.all(bins <= uniform * (1 + 8 * EPS)), name
                got = W.kernel_welch(x, call[0], call[1], nperseg, nperseg - call[2], taper, call[4], cdt)
                r = _ratio(got, tot, bins)
                assert r <= 1, (name, call[2:], cdt, r)
                worst[np.dtype(cdt).name] = max(worst.get(np.dtype(cdt).name, 0.0), r)
                if shares is not None:
                    want = shares[call[4]] if cdt is np.float32 else (W.SHARE_F64,) * x.shape[1]
                    assert np.all((bins < tot).mean(axis=0) >= np.array(want)), (name, call[4], cdt, (bins < tot).mean(axis=0))
    print('nperseg %d: restatement, largest error / per-bin bound %s' % (nperseg, worst))


@pytest.mark.parametrize('cdt', CDTS)
@pytest.mark.parametrize('nperseg', NPERSEG)
def test_block_cases_every_segment_above_the_bound(nperseg, cdt):
    x, channels = W.block_case(cdt, nperseg)
    x = x[:, channels[-3:]]
    n_seg = x.shape[0] // nperseg
    assert n_seg > 2 * W.B and n_seg % W.B
    taper, tot, bins, uniform = _ref(x, (0, x.shape[0], 0, 'boxcar', False), nperseg, cdt)
    assert np.all(bins <= uniform * (1 + 8 * EPS))
    assert float(np.abs(x.astype(np.float64)).reshape(n_seg, nperseg, x.shape[1]).max(axis=1).min()) ** 2 > bins.max()
    got = W.kernel_welch(x, 0, x.shape[0], nperseg, nperseg, taper, False, cdt)
    assert _ratio(got, tot, bins) <= 1


def _mutant_ratios(nperseg, cdt, mutant):
    """{case: (error / per-bin bound, error / uniform bound)} of a mutant of the restatement, worst bin."""
    out = {}
    if mutant == 'seg31':
        x, channels = W.block_case(cdt, nperseg)
        cases = [('blocks', x[:, channels[-2:]], [(0, x.shape[0], 0, 'boxcar', False)], None)]
    else:
        cases = W.edge_cases(nperseg)
    for name, x, calls, _ in cases:
        for i, call in enumerate(calls):
            if mutant == 'mean32' and not (name.startswith('offset') and call[4]):
                continue
            if mutant == 'taper' and isinstance(call[3], str):
                continue
            taper, tot, bins, uniform = _ref(x, call, nperseg, cdt)
            got = W.kernel_welch(x, call[0], call[1], nperseg, nperseg - call[2], taper, call[4], cdt, mutant)
            out['%s/%d' % (name, i)] = (_ratio(got, tot, bins), _ratio(got, tot, uniform))
    return out


@pytest.mark.parametrize('nperseg', [256, 1024, 4096, 16384])
@pytest.mark.parametrize('mutant', ['taper', 'row', 'seg31', 'split_tw', 'mean32'])
def test_mutants_of_the_restatement(mutant, nperseg):
    for cdt in CDTS:
        r = _mutant_ratios(nperseg, cdt, mutant)
        new = max(v[0] for v in r.values())
        old = max(v[1] for v in r.values())
        seen_old = sum(v[1] > 1 for v in r.values())
        print('%-8s nperseg %5d %s: largest error / per-bin bound %.3g (over it in %d of %d cases), / uniform bound %.3g (%s, over it in %d)'
              % (mutant, nperseg, np.dtype(cdt).name, new, sum(v[0] > 1 for v in r.values()), len(r), old,
                 'passed by welch_bound' if old <= 1 else 'failed by welch_bound', seen_old))
        if mutant in ('taper', 'row', 'seg31'):
            assert new > 1, (mutant, nperseg, cdt, r)
        elif mutant == 'split_tw':
            # one bin's twiddle turned by 2 pi / N: 182, 15.4 and 1.64 times the float32 bound at 256, 1024 and 4096, and 0.165 of it at
            # 16384, where the turn (3.8e-4) is below delta sqrt(N E) / |X_k| on every signal here: seen only up to 4096 in float32
            assert new > 1 or (cdt is np.float32 and nperseg == 16384), (mutant, nperseg, cdt, r)
        elif cdt is np.float64:
            assert new > 1, (mutant, nperseg, cdt, r)
        else:
            # float32: the mean's rounding to float32 is of the size of the rounding of x - m to float32 itself, which delta allows
            assert new <= 1, (mutant, nperseg, cdt, r)
