"""Randomised parity of Reader.detect on a GPU box: random recordings (all ten item types, channel counts, chunk durations; float
data with NaN, infinities and zeros of both signs sprinkled in; coarse integers for heavy ties) compressed with mtscomp_amd.compress
and read back with random taps, exclude, spread, sign, reference, thresholds (a scalar or one per column; now and then so low that
most samples are events), ranges, column lists (any order, repeats; up to 1024 columns under a median, so that its sorting network
takes every size up to 1024) and cache states (a random prefix read so that some chunks are resident).  Each case also draws the
decode pieces (MTS_PIPE_BYTES), the slab bound (MTS_DETECT_SLAB_BYTES), one lane or two on device 0, DETECT_CALL_BYTES and the first
buffer's size.
Every comparison is exact: sample, channel and amplitude byte for byte against tests/detect_oracle.py over the oracle's decode.

    python tools/fuzz_detect_gpu.py [seed] [seconds]
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
from tests.detect_oracle import SIGNS, detect_events, filtered  # noqa: E402

MAX_SAMPLES = 12000 * 130
DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


def _env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)


def one_case(rs, tmp):
    dt = np.dtype(DTYPES[rs.randint(len(DTYPES))])
    nc = int(rs.choice([1, 2, 3, 17, 64, 65, 70, 130, 257, 600, 1024]))
    rows = int(rs.randint(1, min(12000, MAX_SAMPLES // nc + 1)))                # (the wide ones are short: a case costs what a 130-column one does)
    _env('MTS_PIPE_BYTES', [None, 64 << 10, 300 << 10, 8 << 20][rs.randint(4)])
    _env('MTS_DETECT_SLAB_BYTES', [None, 1, 40 << 10, 1 << 20][rs.randint(4)])
    api.DETECT_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
    api.DETECT_GUESS_MIN, api.DETECT_GUESS_SAMPLES = [(4096, 256), (1, 1 << 40), (50, 4096)][rs.randint(3)]
    do_time_diff = bool(rs.randint(2))
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 10 ** rs.uniform(-2, 4)).astype(dt)
        if rs.randint(2):
            x = np.round(x / (np.abs(x).max() + 1e-30) * 4).astype(dt)          # five values: ties everywhere
        if rs.randint(2):
            do_time_diff = False                                   # (a float time diff does not keep these bit for bit)
            for v in (np.nan, np.inf, -np.inf, -0.0):
                x[rs.randint(rows, size=2), rs.randint(nc, size=2)] = v
    else:
        info = np.iinfo(dt)
        span = int(10 ** rs.uniform(0.3, 18))
        x = rs.randint(max(info.min, -2 ** 62, -span), min(info.max, 2 ** 62, span) + 1, size=(rows, nc), dtype=np.int64).astype(dt)
    raw = tmp / 'f.bin'
    x.tofile(raw)
    rate = float(rs.choice([1000., 2500., 30000.]))
    cd = float(rs.choice([0.01, 0.1, 0.37])) * 30000. / rate
    mtscomp_amd.compress(raw, tmp / 'f.cbin', tmp / 'f.ch', sample_rate=rate, n_channels=nc, dtype=dt, chunk_duration=cd,
                         do_time_diff=do_time_diff, do_spatial_diff=bool(rs.randint(2)) and dt.kind != 'f', check_after_compress=False)
    ro = mtscomp_amd.decompress(tmp / 'f.cbin', tmp / 'f.ch', codec=OracleCodec(), check_after_decompress=False)
    dec = ro[:]
    ro.close()
    r = mtscomp_amd.decompress(tmp / 'f.cbin', tmp / 'f.ch', codec=api.HipCodec(devices=[0] * int(rs.randint(1, 3))),
                               check_after_decompress=False)
    if rs.randint(2):
        r[:int(rs.randint(1, rows + 1))]                           # some chunks resident
    for _ in range(4):
        start = int(rs.randint(0, rows))
        stop = max(start, int(rs.randint(start, rows + 1)))
        cols = [int(c) for c in rs.randint(0, nc, size=rs.randint(1, 2 * nc + 2))]
        L = int(rs.choice([1, 1, 2, 3, 9, 64, 65, 300]))
        taps = None if L == 1 and rs.randint(2) else rs.randn(L) / np.sqrt(L)
        R = int(rs.choice([0, 1, 2, 7, 30, 255]))
        S = int(rs.choice([0, 1, 3, 32]))
        sign = ['neg', 'pos', 'both'][rs.randint(3)]
        reference = [None, 'median'][rs.randint(2)]
        if reference:
            cols = cols[:1024]
        dense = rs.randint(8) == 0                                 # most samples above the threshold: the compaction at full density
        if dense:
            R, S = min(R, 2), min(S, 1)                            # (the oracle pays per candidate and neighbour)
        xs = dec[:, cols]
        t = np.array([1.0]) if taps is None else taps
        y = filtered(xs, 0, 0, rows, 0, rows, t).astype(np.float64)
        fin = y[np.isfinite(y)]
        scale = float(fin.std()) if fin.size and fin.std() > 0 else 1.0
        scale = min(max(scale, 1e-30), 1e30)
        thr = scale * (1e-3 if dense else float(rs.choice([0.2, 1.0, 2.0])))
        if rs.randint(2):
            thr = thr * rs.uniform(0.5, 2.0, size=len(cols))
        got = r.detect(thr, start, stop, channels=cols, taps=taps, sign=sign, reference=reference, exclude=R, spread=S)
        want = detect_events(xs, 0, 0, rows, start, stop, t, thr, SIGNS[sign], 1 if reference else 0, R, S)
        assert got.sample.tobytes() == want[0].tobytes(), ('sample', got.sample.size, want[0].size, got.sample[:6], want[0][:6])
        assert got.channel.tobytes() == np.asarray(cols, np.int64)[want[1]].tobytes(), 'channel'
        assert got.amplitude.tobytes() == want[2].tobytes(), 'amplitude'
    r.close()


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261018))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 5))
    print('fuzz_detect_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
    t_end = time.time() + seconds
    n = 0
    with tempfile.TemporaryDirectory() as d:
        while time.time() < t_end:
            rs = np.random.RandomState([seed, n])
            try:
                one_case(rs, Path(d))
            except Exception:
                traceback.print_exc()
                print('FAILED: seed %d case %d' % (seed, n), flush=True)
                return 1
            n += 1
    print('fuzz_detect_gpu: %d cases passed' % n, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
