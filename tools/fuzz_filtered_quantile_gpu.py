"""Randomised parity of Reader.quantile / median / mad with taps= / reference= on a GPU box: random recordings (int16, uint8, int32,
float32; channel counts around the wave width; chunk durations so that chunk boundaries fall anywhere in a workgroup's rows; float data
with NaN, infinities and zeros of both signs sprinkled in) compressed with mtscomp_amd.compress and read back with random filters (1
to 130 taps, odd and even; the median reference on and off), windows, ranges, column lists (any order, repeats), quantiles, methods,
centers and cache states (a random prefix read so that some chunks are resident).  Each case also draws the decode pieces
(MTS_PIPE_BYTES), the slab bound (MTS_ZRANK_SLAB_BYTES, down to a row a slab), one lane or two on device 0, QUANTILE_CALL_BYTES and
QUANTILE_SLAB_BYTES.  Windows x columns are capped per case (a cell costs a 2 KiB histogram).  Every comparison is exact: z is that
of tests/detect_oracle.py, the order statistics are held to np.sort by value, median and mad to numpy (tests/select_oracle.py).

    python tools/fuzz_filtered_quantile_gpu.py [seed] [seconds]
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
from tests.filtered_select_oracle import z_rows  # noqa: E402
from tests.select_oracle import check_quantile, np_mad, np_median, same_values  # noqa: E402

DTYPES = ['int16', 'int16', 'uint8', 'int32', 'float32']
METHODS = ['linear', 'lower', 'higher', 'nearest', 'midpoint']
MAX_CELLS = 6000                                     # windows x columns of one call of the Reader
KNOBS = ('MTS_PIPE_BYTES', 'MTS_ZRANK_SLAB_BYTES')


def one_case(rs, tmp):
    dt = np.dtype(DTYPES[rs.randint(len(DTYPES))])
    nc = int(rs.choice([1, 3, 17, 64, 70]))
    rows = int(rs.randint(1, 14000))
    for name, values in zip(KNOBS, ([None, 64 << 10, 300 << 10, 8 << 20], [None, 1, 4 * nc * 7, 4 * nc * 1000, 4 * nc * 4097])):
        v = values[rs.randint(len(values))]
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
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
        kind = rs.randint(3)
        if kind == 0:                                              # few distinct values: heavy ties, constant columns
            x = np.array([info.min, info.max, 0, 1, 7], dtype=dt)[rs.randint(5, size=(rows, nc))]
            x[:, rs.randint(nc)] = 7
        else:
            span = int(10 ** rs.uniform(0.5, 9))
            x = rs.randint(max(info.min, -span), min(info.max, span) + 1, size=(rows, nc), dtype=np.int64).astype(dt)
    raw = tmp / 'f.bin'
    x.tofile(raw)
    rate = float(rs.choice([1000., 2500., 30000.]))
    cd = float(rs.choice([0.01, 0.1, 0.37, 1.0])) * 30000. / rate
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
        n_taps = int(rs.choice([1, 2, 3, 8, 31, 101, 130]))
        taps = None if n_taps == 1 and rs.randint(2) else rs.randn(n_taps) / np.sqrt(n_taps)
        reference = 'median' if taps is None or rs.randint(2) else None
        start = int(rs.randint(0, rows))
        stop = max(int(rs.randint(start, rows + 1)), start)
        n = stop - start
        cols = list(rs.randint(0, nc, size=rs.randint(1, 2 * nc + 2)))
        window = [None, 1, int(rs.randint(1, 50)), int(rs.randint(1, 5000)), 4096, n + int(rs.randint(1, 10))][rs.randint(6)]
        if window is not None and -(-n // window) * len(cols) > MAX_CELLS:      # the cap: fewer rows, same window
            stop = start + window * max(MAX_CELLS // len(cols), 1)
            n = stop - start
        n_win = -(-n // (window or max(n, 1)))
        q = sorted(set([float(rs.choice([0, 0.5, 1, rs.rand()])) for _ in range(rs.randint(1, 4))]))
        method = METHODS[rs.randint(5)]
        z = np.zeros((rows, len(cols)), np.float32)
        z[start:stop] = z_rows(dec[:, cols], 0, 0, rows, start, stop, [1.0] if taps is None else taps, 1 if reference else 0)
        kw = dict(channels=cols, window=window, taps=taps, reference=reference)
        what = rs.randint(4)
        if what == 0:
            got = r.quantile(q, start, stop, method=method, **kw)
            check_quantile(got, z, start, stop, window, q, method)
        elif what == 1:
            cen = rs.randn(n_win, len(cols)) * 10 ** rs.uniform(-1, 3) if rs.randint(2) else float(rs.randn())
            mode = int(rs.randint(1, 3))
            got = r.quantile(q, start, stop, method=method, center=cen, absolute=mode == 2, **kw)
            check_quantile(got, z, start, stop, window, q, method, mode=mode, center=cen)
        elif what == 2:
            assert same_values(r.median(start, stop, **kw), np_median(z, start, stop, window))
        else:
            got = r.mad(start, stop, **kw)
            assert same_values(got.mad, np_mad(z, start, stop, window)) and same_values(got.center, np_median(z, start, stop, window))
    r.close()


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261021))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 30))
    print('fuzz_filtered_quantile_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
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
    print('fuzz_filtered_quantile_gpu: %d cases passed' % n, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
