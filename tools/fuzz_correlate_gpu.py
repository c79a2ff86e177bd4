"""Randomised parity of Reader.correlate on a GPU box: random recordings (all ten item types, channel counts, chunk durations; float
data with NaN, infinities and zeros of both signs sprinkled in, or at the 1e-20 scale whose products are subnormal) compressed with
mtscomp_amd.compress and read back with random templates (1 .. 256 rows, 1 .. 200 of them, zero entries sprinkled in, `before` anywhere
in [0, T]), row ranges (the first and the last row, single rows, ranges off every tile), taps, reference, column lists (any order,
repeats) and cache states (a random prefix read so that some chunks are resident).  Each case also draws the decode pieces
(MTS_PIPE_BYTES), the slab bound (MTS_CORRELATE_SLAB_BYTES), one lane or two on device 0, CORRELATE_CALL_BYTES and CORRELATE_OUT_BYTES.
Every comparison is exact: the scores byte for byte against tests/correlate_oracle.py over the oracle's decode.

    python tools/fuzz_correlate_gpu.py [seed] [seconds]
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
from tests.correlate_oracle import correlate  # noqa: E402

MAX_STEPS = 3000                                                   # fmaf passes of the oracle per call: columns (padded) x T ...
MAX_SCORES = 20000                                                 # ... each over this many scores at most
DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


def _env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)


def one_case(rs, tmp):
    dt = np.dtype(DTYPES[rs.randint(len(DTYPES))])
    nc = int(rs.choice([1, 2, 3, 5, 17, 64, 65, 70, 130, 385]))
    rows = int(rs.randint(1, 3000))
    _env('MTS_PIPE_BYTES', [None, 64 << 10, 300 << 10, 8 << 20][rs.randint(4)])
    do_time_diff = bool(rs.randint(2))
    scale = 1.0
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 10 ** rs.uniform(-2, 4)).astype(dt)
        kind = rs.randint(3)
        if kind == 1:
            do_time_diff = False                                   # (a float time diff does not keep these bit for bit)
            for v in (np.nan, np.inf, -np.inf, -0.0):
                x[rs.randint(rows, size=2), rs.randint(nc, size=2)] = v
        elif kind == 2 and dt == np.float32:
            x = (rs.randn(rows, nc) * 1e-20).astype(dt)
            scale = 1e-20
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
    for _ in range(3):
        n_cols = int(rs.randint(1, min(2 * nc + 2, 400)))
        cols = [int(c) for c in rs.randint(0, nc, size=n_cols)]
        n4 = -(-n_cols // 4) * 4
        T = int(min(rs.choice([1, 2, 3, 16, 17, 61, 256, int(rs.randint(1, 257))]), max(1, MAX_STEPS // n4)))
        before = int([0, T, min(20, T), int(rs.randint(0, T + 1))][rs.randint(4)])
        K = int(rs.choice([1, 2, 15, 16, 17, 64, 65, int(rs.randint(1, 200))]))
        L = int(rs.choice([1, 1, 2, 3, 9, 64, 65, 300]))
        taps = None if L == 1 and rs.randint(2) else rs.randn(L) / np.sqrt(L)
        reference = [None, 'median'][rs.randint(2)]
        k = rs.randn(K, T, n_cols) * scale
        k[rs.randint(0, K, 20), rs.randint(0, T, 20), rs.randint(0, n_cols, 20)] = 0.0
        span = max(1, min(rows, MAX_SCORES // K))
        i0 = int([0, max(0, rows - span), int(rs.randint(0, rows))][rs.randint(3)])
        i1 = int(min(rows, i0 + [span, 1, int(rs.randint(1, span + 1))][rs.randint(3)]))
        _env('MTS_CORRELATE_SLAB_BYTES', [None, 1, 4 * n_cols * (T + 70), 1 << 20][rs.randint(4)] if i1 - i0 <= 600 else [None, 1 << 20][rs.randint(2)])
        api.CORRELATE_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
        api.CORRELATE_OUT_BYTES = [4 * K * 37, 1 << 16, 1 << 30][rs.randint(3)]
        got = r.correlate(k, i0, i1, channels=cols, before=before, taps=taps, reference=reference)
        want = correlate(dec[:, cols], 0, 0, rows, i0, i1, [1.0] if taps is None else taps, 1 if reference else 0, before, k)
        assert got.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape)
        assert got.tobytes() == want.tobytes(), ('scores', got.shape, T, before, n_cols, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    r.close()


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261019))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 5))
    print('fuzz_correlate_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
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
    print('fuzz_correlate_gpu: %d cases passed' % n, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
