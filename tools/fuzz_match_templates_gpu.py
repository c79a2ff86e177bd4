"""Randomised parity of Reader.match_templates on a GPU box: random recordings (all ten item types, channel counts, chunk durations;
float data with NaN, infinities and zeros of both signs sprinkled in, or quantised so that scores tie) compressed with
mtscomp_amd.compress and read back with random templates (1 .. 256 rows, 1 .. 200 of them, copies of one another among them, `before`
anywhere in [0, T]), thresholds (a percentile of the oracle's scores per template, or so low that every row is a candidate),
exclusion radii (0 .. 255), row ranges (the first and the last row, single rows, ranges off every word of the bitmap), taps, reference,
column lists (any order, repeats) and cache states (a random prefix read so that some chunks are resident).  Each case also draws the
decode pieces (MTS_PIPE_BYTES), the slab bound (MTS_TMATCH_SLAB_BYTES), one lane or two on device 0, TMATCH_CALL_BYTES and the first
buffer's size.  Every comparison is exact: the events byte for byte against tests/tmatch_oracle.py over the oracle's decode.

    python tools/fuzz_match_templates_gpu.py [seed] [seconds]
"""
import os
import sys
import tempfile
import time
import traceback
import warnings
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import mtscomp_amd  # noqa: E402
from mtscomp_amd import api  # noqa: E402
from tests.codec_oracle import OracleCodec  # noqa: E402
from tests.correlate_oracle import correlate  # noqa: E402
from tests.tmatch_oracle import events_of_scores  # noqa: E402

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
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 10 ** rs.uniform(-2, 4)).astype(dt)
        kind = rs.randint(3)
        if kind == 1:
            do_time_diff = False                                   # (a float time diff does not keep these bit for bit)
            for v in (np.nan, np.inf, -np.inf, -0.0):
                x[rs.randint(rows, size=2), rs.randint(nc, size=2)] = v
        elif kind == 2:
            do_time_diff = False
            x = np.round(rs.randn(rows, nc)).astype(dt)            # few values: equal scores within rows and between them
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
        k = rs.randn(K, T, n_cols)
        if rs.randint(2):
            k = np.round(k)                                        # (with quantised data: exact ties)
        for _ in range(rs.randint(0, 4)):
            k[rs.randint(K)] = k[rs.randint(K)]                    # identical templates
        R = int([0, 1, 2, 63, 64, 255, int(rs.randint(0, 256))][rs.randint(7)])
        span = max(1, min(rows, MAX_SCORES // K))
        i0 = int([0, max(0, rows - span), int(rs.randint(0, rows))][rs.randint(3)])
        i1 = int(min(rows, i0 + [span, 1, int(rs.randint(1, span + 1))][rs.randint(3)]))
        a, b = max(0, i0 - R), min(rows, i1 + R)                   # the oracle scores every row the events read
        if (b - a) * K > 3 * MAX_SCORES:
            R = 2
            a, b = max(0, i0 - R), min(rows, i1 + R)
        score = correlate(dec[:, cols], 0, 0, rows, a, b, [1.0] if taps is None else taps, 1 if reference else 0, before, k)
        with np.errstate(invalid='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')                        # (a column of scores without a finite one)
            pct = np.nanpercentile(np.where(np.isfinite(score), score, np.nan), [50, 90, 99][rs.randint(3)], axis=0)
        thr = [np.where(np.isfinite(pct), pct, 0.0).astype(np.float32), np.float32(-3e38), np.float32(0.0)][rs.randint(3)]
        z_row, s_row = 4 * n_cols, 4 * K
        some = max(z_row * (2 * R + T + 70), s_row * (2 * R + 70))
        _env('MTS_TMATCH_SLAB_BYTES', [None, 1, some, 1 << 20][rs.randint(4)] if i1 - i0 <= 600 else [None, 1 << 20][rs.randint(2)])
        api.TMATCH_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
        api.TMATCH_GUESS_MIN = [1, 16, 4096][rs.randint(3)]
        got = r.match_templates(k, thr, i0, i1, channels=cols, before=before, taps=taps, reference=reference, exclude=R)
        want = events_of_scores(score, a, i0, i1, thr, R)
        what = (T, before, n_cols, K, R, i0, i1)
        assert (got.sample.dtype, got.template.dtype, got.score.dtype) == (np.int64, np.int64, np.float32)
        assert got.sample.tobytes() == want[0].tobytes(), ('rows', what, got.sample[:6], want[0][:6])
        assert got.template.tobytes() == want[1].tobytes(), ('templates', what, got.template[:6], want[1][:6])
        assert got.score.tobytes() == want[2].tobytes(), ('scores', what)
    r.close()


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261019))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 5))
    print('fuzz_match_templates_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
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
    print('fuzz_match_templates_gpu: %d cases passed' % n, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
