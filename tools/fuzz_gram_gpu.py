"""Randomised parity of Reader.cov on a GPU box: random recordings (all ten item types, channel counts, chunk durations, time /
spatial diff) compressed with mtscomp_amd.compress and read back through Reader.cov with random windows, ranges, column lists
(any order, repeats), ddof and cache states (a random prefix read so that some chunks are resident).  Each case also draws the decode
pieces (MTS_PIPE_BYTES, read by the library at every call: 64 KiB to 8 MiB, or the default), one lane or two on device 0, and
GRAM_CALL_BYTES; one case in four is a long recording of 1.1 to 2.3 M rows and few channels, so that a window holds several groups and
calls and lanes start after the first one.  Exact types are compared with numpy int64 bit for bit, the others with the longdouble
reference within gram_bound (tests/gram_oracle.py: check_cov_result; the bound's teeth are asserted by the fixed cases of
tests/test_gpu_gram.py, not here: random data may hold a row of near-zero items that no bound of this form can see).

    python tools/fuzz_gram_gpu.py [seed] [seconds]
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
from tests.gram_oracle import check_cov_result  # noqa: E402

DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


def one_case(rs, tmp):
    dt = np.dtype(DTYPES[rs.randint(len(DTYPES))])
    long_case = rs.randint(4) == 0
    nc = int(rs.choice([1, 2, 3])) if long_case else int(rs.choice([1, 3, 17, 40, 70]))
    rows = int(rs.randint(1_100_000, 2_300_000)) if long_case else int(rs.randint(1, 30000))
    pipe = [None, 64 << 10, 300 << 10, 1 << 20, 8 << 20][rs.randint(5)]
    if pipe is None:
        os.environ.pop('MTS_PIPE_BYTES', None)
    else:
        os.environ['MTS_PIPE_BYTES'] = str(pipe)
    api.GRAM_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 10 ** rs.uniform(-2, 4) + rs.uniform(-100, 100, size=nc) * 10 ** rs.uniform(0, 3)).astype(dt)
    else:
        info = np.iinfo(dt)
        lo, hi = max(info.min, -2 ** 40), min(info.max, 2 ** 40)
        if rs.randint(3) == 0:                                     # extremes: whole columns at the type's limits
            x = rs.choice([info.min, info.max, 0], size=(1, nc)).repeat(rows, axis=0).astype(dt)
        else:
            x = rs.randint(lo, hi, size=(rows, nc), dtype=np.int64).astype(dt)
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
        r[:int(rs.randint(1, rows + 1))]                               # some chunks resident
    worst = 0.0
    for _ in range(2 if long_case else 4):
        start = int(rs.randint(0, max(rows // 8, 1) if long_case else rows))
        stop = rows - int(rs.randint(0, 1000)) if long_case else int(rs.randint(start, rows + 1))
        stop = max(stop, start)
        n = stop - start
        if long_case:
            window = [None, int(rs.randint(1 << 19, 1 << 21)), int(rs.randint(1000, 300000))][rs.randint(3)]
        else:
            window = [None, 1, int(rs.randint(1, 50)), int(rs.randint(1, 5000)), n + int(rs.randint(0, 10))][rs.randint(5)]
            if window == 0:
                window = None
        cols = list(rs.randint(0, nc, size=rs.randint(1, 2 * nc + 2)))
        ddof = int(rs.randint(0, 3))
        got = r.cov(start, stop, channels=cols, window=window, ddof=ddof)
        worst = max(worst, check_cov_result(got, dec[:, cols], start, stop, window, ddof=ddof, teeth=False))
    r.close()
    return worst


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261016))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 30))
    print('fuzz_gram_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
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
    print('fuzz_gram_gpu: %d cases passed, largest error / allowance %.3g' % (n, worst), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
