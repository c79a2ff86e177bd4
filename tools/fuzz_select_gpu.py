"""Randomised parity of Reader.quantile / median / mad on a GPU box: random recordings (all ten item types, channel counts, chunk
durations, time / spatial diff; float data with NaN, infinities and zeros of both signs sprinkled in, integer columns at the type's
limits) compressed with mtscomp_amd.compress and read back with random windows, ranges, column lists (any order, repeats), quantiles,
methods, centers and cache states (a random prefix read so that some chunks are resident).  Each case also draws the decode pieces
(MTS_PIPE_BYTES), one lane or two on device 0, QUANTILE_CALL_BYTES and QUANTILE_SLAB_BYTES.  Windows x columns are capped per case so
that a case stays within the slab budget (a cell costs a 2 KiB histogram).  Every comparison is exact (tests/select_oracle.py): the
order statistics against np.sort, by value for floats and by bytes for integers; median and mad against numpy.

    python tools/fuzz_select_gpu.py [seed] [seconds]
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
from tests.select_oracle import check_quantile, np_mad, np_median, same_values  # noqa: E402

DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']
METHODS = ['linear', 'lower', 'higher', 'nearest', 'midpoint']
MAX_CELLS = 20000                                    # windows x columns of one call of the Reader


def one_case(rs, tmp):
    dt = np.dtype(DTYPES[rs.randint(len(DTYPES))])
    long_case = rs.randint(5) == 0
    nc = int(rs.choice([1, 2, 3])) if long_case else int(rs.choice([1, 3, 17, 64, 70]))
    rows = int(rs.randint(300_000, 900_000)) if long_case else int(rs.randint(1, 30000))
    pipe = [None, 64 << 10, 300 << 10, 1 << 20, 8 << 20][rs.randint(5)]
    if pipe is None:
        os.environ.pop('MTS_PIPE_BYTES', None)
    else:
        os.environ['MTS_PIPE_BYTES'] = str(pipe)
    api.QUANTILE_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
    api.QUANTILE_SLAB_BYTES = [1, 1 << 20, 1 << 30][rs.randint(3)]
    do_time_diff = bool(rs.randint(2))
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 10 ** rs.uniform(-2, 4) + rs.uniform(-100, 100, size=nc) * 10 ** rs.uniform(0, 3)).astype(dt)
        if rs.randint(2):
            x[rs.rand(rows, nc) < 0.3] = 0
        if rs.randint(2):
            do_time_diff = False                                   # (a float time diff does not keep these bit for bit)
            for v in (np.nan, -np.nan, np.inf, -np.inf, -0.0):
                x[rs.randint(rows, size=3), rs.randint(nc, size=3)] = v
    else:
        info = np.iinfo(dt)
        lo, hi = max(info.min, -2 ** 62), min(info.max, 2 ** 62)
        kind = rs.randint(4)
        if kind == 0:                                              # extremes: whole columns at the type's limits
            x = np.array([info.min, info.max, 0], dtype=dt)[rs.randint(3, size=(1, nc))].repeat(rows, axis=0)
        elif kind == 1:                                            # few distinct values: heavy ties
            x = np.array([info.min, info.max, 0, 1, 7], dtype=dt)[rs.randint(5, size=(rows, nc))]
        else:
            span = int(10 ** rs.uniform(0.5, 18))
            x = rs.randint(max(lo, -span), min(hi, span) + 1, size=(rows, nc), dtype=np.int64).astype(dt)
    raw = tmp / 'f.bin'
    x.tofile(raw)
    rate = float(rs.choice([1000., 2500., 30000.]))
    cd = float(rs.choice([0.01, 0.1, 0.37, 1.0])) * 30000. / rate
    if long_case:
        cd = float(rs.choice([0.5, 1.3, 3.0])) * 30000. / rate
    mtscomp_amd.compress(raw, tmp / 'f.cbin', tmp / 'f.ch', sample_rate=rate, n_channels=nc, dtype=dt, chunk_duration=cd,
                         do_time_diff=do_time_diff, do_spatial_diff=bool(rs.randint(2)) and dt.kind != 'f', check_after_compress=False)
    ro = mtscomp_amd.decompress(tmp / 'f.cbin', tmp / 'f.ch', codec=OracleCodec(), check_after_decompress=False)
    dec = ro[:]
    ro.close()
    r = mtscomp_amd.decompress(tmp / 'f.cbin', tmp / 'f.ch', codec=api.HipCodec(devices=[0] * int(rs.randint(1, 3))),
                               check_after_decompress=False)
    if rs.randint(2):
        r[:int(rs.randint(1, rows + 1))]                           # some chunks resident
    for _ in range(2 if long_case else 4):
        start = int(rs.randint(0, max(rows // 8, 1) if long_case else rows))
        stop = rows - int(rs.randint(0, 1000)) if long_case else int(rs.randint(start, rows + 1))
        stop = max(stop, start)
        n = stop - start
        cols = list(rs.randint(0, nc, size=rs.randint(1, 2 * nc + 2)))
        if long_case:
            window = [None, int(rs.randint(1 << 17, 1 << 19)), int(rs.randint(5000, 300000))][rs.randint(3)]
        else:
            window = [None, 1, int(rs.randint(1, 50)), int(rs.randint(1, 5000)), n + int(rs.randint(1, 10))][rs.randint(5)]
        if window is not None and -(-n // window) * len(cols) > MAX_CELLS:      # the cap: fewer rows, same window
            stop = start + window * max(MAX_CELLS // len(cols), 1)
            n = stop - start
        n_win = -(-n // (window or max(n, 1)))
        q = sorted(set([float(rs.choice([0, 0.5, 1, rs.rand()])) for _ in range(rs.randint(1, 4))]))
        method = METHODS[rs.randint(5)]
        xs = dec[:, cols]
        what = rs.randint(4)
        if what == 0:
            got = r.quantile(q, start, stop, channels=cols, window=window, method=method)
            check_quantile(got, xs, start, stop, window, q, method)
        elif what == 1:
            cen = rs.randn(n_win, len(cols)) * 10 ** rs.uniform(-1, 3) if rs.randint(2) else float(rs.randn())
            mode = int(rs.randint(1, 3))
            got = r.quantile(q, start, stop, channels=cols, window=window, method=method, center=cen, absolute=mode == 2)
            check_quantile(got, xs, start, stop, window, q, method, mode=mode, center=cen)
        elif what == 2:
            assert same_values(r.median(start, stop, channels=cols, window=window), np_median(xs, start, stop, window))
        else:
            got = r.mad(start, stop, channels=cols, window=window)
            assert same_values(got.mad, np_mad(xs, start, stop, window)) and same_values(got.center, np_median(xs, start, stop, window))
    r.close()


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261016))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 30))
    print('fuzz_select_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
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
    print('fuzz_select_gpu: %d cases passed' % n, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
