"""Randomised parity of Reader.welch on a GPU box: random recordings (all ten item types, channel counts, chunk durations, time /
spatial diff) compressed with mtscomp_amd.compress and read back through Reader.welch with random nperseg, noverlap, windows,
detrends, scalings, compute types, ranges, channels and cache states (a random prefix read so that some chunks are resident).
Each case also draws the decode pieces (MTS_PIPE_BYTES, read by the library at every call: 64 KiB to 8 MiB, or the default), one
lane or two on device 0, and WELCH_CALL_BYTES; one case in four is a long recording of 1.1 to 2.6 M rows and few channels, so that
a range holds several groups and calls and lanes start after the first one.  Half the cases draw a structured input instead of white
noise (a tone over noise, an offset with small noise, a random walk, sparse impulses), and array tapers may be negative.  Every result
is compared with welch_f64 over the oracle's decode within welch_bound_bins, the bound per bin.

    python tools/fuzz_welch_gpu.py [seed] [seconds]
"""
import os
import sys
import tempfile
import time
import traceback
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import mtscomp_amd  # noqa: E402
from mtscomp_amd import api  # noqa: E402
from tests.codec_oracle import OracleCodec  # noqa: E402
from tests.welch_oracle import assert_welch_close, psd_scale, welch_bound_bins, welch_f64  # noqa: E402

DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


def structured(rs, rows, nc, dt):
    """A recording whose energy sits in few bins, scaled to the item type's range: a tone over noise 60 dB below, an offset with
    small noise, a random walk, or sparse impulses."""
    if dt.kind == 'f':
        lo, hi = -1e4, 1e4
    else:
        info = np.iinfo(dt)
        lo, hi = float(max(info.min, -2 ** 40)), float(min(info.max, 2 ** 40))
    mid, amp = (lo + hi) / 2, (hi - lo) / 2
    kind = rs.randint(4)
    n = np.arange(rows)[:, None]
    if kind == 0:
        v = mid + 0.8 * amp * (np.sin(n * rs.uniform(0.01, 3.0, size=nc) + rs.uniform(0, 6, size=nc)) + 1e-3 * rs.randn(rows, nc))
    elif kind == 1:
        v = mid + 0.9 * amp * rs.uniform(-1, 1) + 1e-3 * amp * rs.randn(rows, nc)
    elif kind == 2:
        v = np.cumsum(rs.randn(rows, nc), axis=0)
        v = mid + 0.9 * amp * v / np.abs(v).max()
    else:
        v = np.full((rows, nc), mid if dt.kind == 'u' else 0.0)
        hit = rs.rand(rows, nc) < 0.01
        v[hit] += 0.9 * amp * rs.uniform(-1, 1, size=int(hit.sum()))
    v = np.clip(v, lo, hi)
    return (v if dt.kind == 'f' else np.rint(v)).astype(dt)


def one_case(rs, tmp):
    dt = np.dtype(DTYPES[rs.randint(len(DTYPES))])
    long_case = rs.randint(4) == 0
    nc = int(rs.choice([1, 2, 3])) if long_case else int(rs.choice([1, 3, 17, 64, 100]))
    rows = int(rs.randint(1_100_000, 2_600_000)) if long_case else int(rs.randint(300, 40000))
    pipe = [None, 64 << 10, 300 << 10, 1 << 20, 8 << 20][rs.randint(5)]
    if pipe is None:
        os.environ.pop('MTS_PIPE_BYTES', None)
    else:
        os.environ['MTS_PIPE_BYTES'] = str(pipe)
    api.WELCH_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 10 ** rs.uniform(-2, 4) + rs.uniform(-100, 100)).astype(dt)
    else:
        info = np.iinfo(dt)
        lo, hi = max(info.min, -2 ** 40), min(info.max, 2 ** 40)
        x = rs.randint(lo, hi, size=(rows, nc), dtype=np.int64).astype(dt)
    if rs.randint(2):
        x = structured(rs, rows, nc, dt)
    raw = tmp / 'f.bin'
    x.tofile(raw)
    rate = float(rs.choice([1000., 2500., 30000.]))
    cd = float(rs.choice([0.01, 0.1, 0.37, 1.0])) * 30000. / rate
    if long_case:
        cd = float(rs.choice([0.5, 1.3, 3.0])) * 30000. / rate
    mtscomp_amd.compress(raw, tmp / 'f.cbin', tmp / 'f.ch', sample_rate=rate, n_channels=nc, dtype=dt, chunk_duration=cd,
                         do_time_diff=bool(rs.randint(2)), do_spatial_diff=bool(rs.randint(2)) and dt.kind != 'f',
                         check_after_compress=False)
    ro = mtscomp_amd.decompress(tmp / 'f.cbin', tmp / 'f.ch', codec=OracleCodec(), check_after_decompress=False)
    dec = ro[:]
    ro.close()
    r = mtscomp_amd.decompress(tmp / 'f.cbin', tmp / 'f.ch', codec=api.HipCodec(devices=[0] * int(rs.randint(1, 3))),
                               check_after_decompress=False)
    if rs.randint(2):
        r[:int(rs.randint(1, rows))]                                   # some chunks resident
    worst = 0.0
    for _ in range(2 if long_case else 4):
        lg = int(rs.randint(10 if long_case else 4, min(14, int(np.log2(rows))) + 1))
        nperseg = 1 << lg
        start = int(rs.randint(0, rows // 8 if long_case else rows - nperseg + 1))
        stop = rows - int(rs.randint(0, 1000)) if long_case else int(rs.randint(start + nperseg, rows + 1))
        noverlap = ([None, 0, int(rs.randint(nperseg // 2))] if long_case else [None, 0, nperseg - 1, int(rs.randint(nperseg))])[rs.randint(3 if long_case else 4)]
        window = ['hann', 'hamming', 'boxcar', (rs.rand(nperseg) + 0.1) * (rs.choice([-1.0, 1.0], size=nperseg) if rs.randint(2) else 1.0)][rs.randint(4)]
        detrend = ['constant', False][rs.randint(2)]
        scaling = ['density', 'spectrum'][rs.randint(2)]
        cdt = [np.float32, np.float64][rs.randint(2)]
        cols = list(rs.randint(0, nc, size=rs.randint(1, 2 * nc + 2)))
        step = nperseg - (nperseg // 2 if noverlap is None else noverlap)
        if not long_case and (stop - start - nperseg) // step + 1 > 3000:   # (keep the float64 reference quick)
            stop = start + nperseg + 2999 * step
        f, got = r.welch(nperseg, start, stop, channels=cols, noverlap=noverlap, window=window, detrend=detrend, scaling=scaling, dtype=cdt)
        taper = api.welch_window(window, nperseg)
        tot, _, n_seg, first = welch_f64(dec[:, cols], start, stop, nperseg, step, taper, detrend == 'constant', cdt)
        k = psd_scale(nperseg, taper, scaling, rate, n_seg)[:, None]
        worst = max(worst, assert_welch_close(got, tot * k, welch_bound_bins(tot, first, n_seg) * k))
    r.close()
    return worst


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261016))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 30))
    print('fuzz_welch_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
    t_end = time.time() + seconds
    n, worst = 0, 0.0
    with tempfile.TemporaryDirectory() as d:
        while time.time() < t_end:
            rs = np.random.RandomState([seed, n])
            try:
                worst = max(worst, one_case(rs, Path(d)))
            except Exception:
                traceback.print_exc()
                print('FAILED: seed %d case %d' % (seed, n), flush=True)
                return 1
            n += 1
    print('fuzz_welch_gpu: %d cases passed, largest error / bound %.3g' % (n, worst), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
