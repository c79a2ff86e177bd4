"""Randomised parity of Reader.project on a GPU box: random recordings (all ten item types, channel counts, chunk durations; float
data with NaN, infinities and zeros of both signs sprinkled in) compressed with mtscomp_amd.compress and read back with random
weights (dense, sparse, dyadic; now and then tiny, so that float32 products are subnormal), offsets (none, a scalar, one per column),
column lists (any order, repeats, up to 1024), output counts up to 1024, ranges and cache states (a random prefix read so that some
chunks are resident).  Each case also draws the decode pieces (MTS_PIPE_BYTES), one lane or two on device 0, PROJECT_CALL_BYTES and
PROJECT_OUT_BYTES.
The two acceptance rules of tests/test_gpu_project.py: float32 bit for bit the fmaf chain of tests/project_oracle.py over the
oracle's decode (NaN as NaN); float64 within project_bound of the longdouble reference where that is finite, on rows without NaN or
infinities, and with the NaN pattern of the float64 chain elsewhere.

    python tools/fuzz_project_gpu.py [seed] [seconds]
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
from tests.project_oracle import assert_project_within, assert_same_bits, project_chain_f32, project_chain_f64  # noqa: E402

MAX_WORK = 6000 * 64 * 64                                          # rows * columns * outputs of a case: what the numpy chain costs
DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


def _env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)


def one_case(rs, tmp):
    dt = np.dtype(DTYPES[rs.randint(len(DTYPES))])
    nc = int(rs.choice([1, 2, 3, 17, 64, 65, 70, 130, 385, 1024]))
    n_cols = int(rs.choice([1, 2, 3, 4, 5, 31, 33, 63, 64, 65, 127, 129, 385, 1024]))
    n_out = int(rs.choice([1, 2, 8, 15, 16, 17, 63, 64, 65, 130, 385, 1024]))
    rows = int(rs.randint(1, max(2, min(6000, MAX_WORK // (n_cols * n_out) + 1))))
    _env('MTS_PIPE_BYTES', [None, 64 << 10, 300 << 10, 8 << 20][rs.randint(4)])
    api.PROJECT_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
    api.PROJECT_OUT_BYTES = [1 << 12, 1 << 20, 1 << 30][rs.randint(3)]
    do_time_diff = bool(rs.randint(2))
    special = False
    tiny = dt == np.float32 and rs.randint(4) == 0
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * (1e-20 if tiny else 10 ** rs.uniform(-2, 4))).astype(dt)
        if rs.randint(2):
            do_time_diff = False                                   # (a float time diff does not keep these bit for bit)
            special = True
            for v in (np.nan, np.inf, -np.inf, -0.0):
                x[rs.randint(rows, size=2), rs.randint(nc, size=2)] = v
    else:
        info = np.iinfo(dt)
        span = int(10 ** rs.uniform(0.3, 18))
        x = rs.randint(max(info.min, -2 ** 62, -span), min(info.max, 2 ** 62, span) + 1, size=(rows, nc), dtype=np.int64).astype(dt)
    raw = tmp / 'f.bin'
    x.tofile(raw)
    rate = float(rs.choice([1000., 2500., 30000.]))
    cd = float(rs.choice([0.003, 0.01, 0.1])) * 30000. / rate
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
        start = int(rs.randint(0, rows))
        stop = int(rs.randint(start, rows + 1))
        cols = [int(c) for c in rs.randint(0, nc, size=n_cols)]
        kind = rs.randint(3)
        w = rs.randn(n_cols, n_out) if kind == 0 else rs.randn(n_cols, n_out) * (rs.rand(n_cols, n_out) < 0.2) if kind == 1 else \
            rs.randint(-8, 9, size=(n_cols, n_out)) / 16.0
        if tiny:
            w = w * 1e-20
        scale = 1e-21 if tiny else float(np.abs(dec[np.isfinite(dec)]).max()) if np.isfinite(dec).any() else 1.0
        off = [None, float(rs.randn() * scale), rs.randn(n_cols) * scale][rs.randint(3)]
        xs = dec[start:stop][:, cols]
        got = r.project(w, start, stop, channels=cols, offset=off, dtype=np.float32)
        assert_same_bits(got, project_chain_f32(xs, off, w))
        if tiny:
            continue                                               # (float32 subnormals: nothing new in float64)
        got = r.project(w, start, stop, channels=cols, offset=off, dtype=np.float64)
        fin = np.isfinite(xs.astype(np.float64)).all(axis=1) if special else np.ones(xs.shape[0], bool)
        if fin.any():
            assert_project_within(got[fin], xs[fin], off, w, np.float64)
        if special and not fin.all():
            assert np.array_equal(np.isnan(got[~fin]), np.isnan(project_chain_f64(xs[~fin], off, w))), 'NaN pattern'
    r.close()


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261018))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 5))
    print('fuzz_project_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
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
    print('fuzz_project_gpu: %d cases passed' % n, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
