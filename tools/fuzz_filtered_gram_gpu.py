"""Randomised parity of Reader.cov with taps= / reference= on a GPU box: random recordings (int16, uint8, int32, float32; channel counts
around the super tile of 64 columns and with every n_cols % 4; chunk durations so that chunk boundaries fall anywhere in a Gram slab;
float data with NaN, infinities and zeros sprinkled in) compressed with mtscomp_amd.compress and read back with random filters (1 to
130 taps, odd and even; the median reference on and off), windows, ranges, column lists (any order, repeats) and cache states (a random
prefix read so that some chunks are resident).  Each case also draws the decode pieces (MTS_PIPE_BYTES), the z-slab bound
(MTS_ZGRAM_SLAB_BYTES, down to one Gram slab), one lane or two on device 0, GRAM_CALL_BYTES and GRAM_SLAB_BYTES.  Two comparisons per
call: bit for bit (NaN places, every other bit) against cov of a float32 recording that holds z -- residual([], ...) of the same
Reader, written and compressed --, which runs k_gram<float> and k_gram_colsum on the same items; and gram_oracle.check_cov_result on the
z of tests/filtered_select_oracle.py (the bound of include/mtscomp_hip.h, NaN and infinities where the float64 reference has them).

    python tools/fuzz_filtered_gram_gpu.py [seed] [seconds]
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
from tests.gram_oracle import assert_order_free, check_cov_result  # noqa: E402

DTYPES = ['int16', 'int16', 'uint8', 'int32', 'float32']
MAX_BYTES = 64 << 20                                 # of the Gram matrices of one call of the Reader
KNOBS = ('MTS_PIPE_BYTES', 'MTS_ZGRAM_SLAB_BYTES')


def same_bits(got, want):
    for key in ('gram', 'sum'):
        a, b = got[key], want[key]
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape, key
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb), key + ': NaN places'
        assert a[~na].tobytes() == b[~nb].tobytes(), key
    assert got.count.tolist() == want.count.tolist()


def one_case(rs, tmp):
    dt = np.dtype(DTYPES[rs.randint(len(DTYPES))])
    nc = int(rs.choice([1, 2, 3, 17, 64, 70]))
    rows = int(rs.randint(1, 14000))
    for name, values in zip(KNOBS, ([None, 64 << 10, 300 << 10, 8 << 20], [None, 1, 4 * nc * 4096, 4 * nc * 4096 * 2 + 5])):
        v = values[rs.randint(len(values))]
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
    api.GRAM_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
    api.GRAM_SLAB_BYTES = [1, 1 << 20, 1 << 30][rs.randint(3)]
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
    for _ in range(2):
        n_taps = int(rs.choice([1, 2, 3, 8, 31, 101, 130]))
        taps = None if n_taps == 1 and rs.randint(2) else rs.randn(n_taps) / np.sqrt(n_taps)
        reference = 'median' if taps is None or rs.randint(2) else None
        cols = list(rs.randint(0, nc, size=rs.randint(1, 2 * nc + 2)))
        # z from the device as a float32 recording of its own: the existing kernels on the same items
        zf = r.residual([], [], [], np.zeros((1, 1, len(cols)), np.float32), channels=cols, before=0, taps=taps, reference=reference)
        zo = z_rows(dec[:, cols], 0, 0, rows, 0, rows, [1.0] if taps is None else taps, 1 if reference else 0)
        assert zf.tobytes() == zo.tobytes()
        zf.tofile(tmp / 'z.bin')
        mtscomp_amd.compress(tmp / 'z.bin', tmp / 'z.cbin', tmp / 'z.ch', sample_rate=rate, n_channels=len(cols), dtype=np.float32,
                             chunk_duration=cd, do_time_diff=False, check_after_compress=False)
        rz = mtscomp_amd.decompress(tmp / 'z.cbin', tmp / 'z.ch', check_after_decompress=False)
        for _ in range(3):
            start = int(rs.randint(0, rows))
            stop = max(int(rs.randint(start, rows + 1)), start)
            n = stop - start
            window = [None, 1, int(rs.randint(1, 50)), int(rs.randint(1, 5000)), 4096, n + int(rs.randint(1, 10))][rs.randint(6)]
            cell = 8 * len(cols) * len(cols)
            if window is not None and -(-n // window) * cell > MAX_BYTES:          # the cap: fewer rows, same window
                stop = start + window * max(MAX_BYTES // cell, 1)
            ddof = int(rs.randint(3))
            got = r.cov(start, stop, channels=cols, window=window, ddof=ddof, taps=taps, reference=reference)
            same_bits(got, rz.cov(start, stop, window=window, ddof=ddof))
            if stop == start:
                continue
            try:
                assert_order_free(zo, start, stop, window)
            except AssertionError:
                continue                                           # (the order of the sum decides an entry: no reference can say which)
            check_cov_result(got, zo, start, stop, window, ddof=ddof, teeth=False)
        rz.close()
    r.close()


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261021))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 30))
    print('fuzz_filtered_gram_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
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
    print('fuzz_filtered_gram_gpu: %d cases passed' % n, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
