"""Randomised parity of Reader.residual and Reader.match_templates(subtract=) on a GPU box: random recordings (all ten item types,
channel counts, chunk durations; float data with NaN, infinities and zeros of both signs sprinkled in) compressed with
mtscomp_amd.compress and read back with random templates (1 .. 256 rows, `before` anywhere in [0, T]) and random event lists: empty,
sparse, clustered tens deep on a few rows, with ties, at the first and the last sample, in any order, amplitudes of both signs, zero,
tiny and huge.  Each case also draws the row range, taps, reference, column list (any order, repeats; widths on and off the vector
path), cache state, the decode pieces (MTS_PIPE_BYTES), the slab bounds (MTS_RESIDUAL_SLAB_BYTES, MTS_TMATCH_SLAB_BYTES), one lane or
two on device 0 and the call cuts.  Every comparison is exact: the rows and the events byte for byte against tests/residual_oracle.py
over the oracle's decode.

    python tools/fuzz_residual_gpu.py [seed] [seconds]
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
from tests.residual_oracle import match_residual, residual  # noqa: E402

MAX_STEPS = 3000                                                   # fmaf passes of the oracle's scores per call: columns (padded) x T
DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


def _env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)


def one_case(rs, tmp):
    dt = np.dtype(DTYPES[rs.randint(len(DTYPES))])
    nc = int(rs.choice([1, 2, 3, 4, 5, 17, 64, 65, 130, 385]))
    rows = int(rs.randint(1, 2500))
    _env('MTS_PIPE_BYTES', [None, 64 << 10, 300 << 10, 8 << 20][rs.randint(4)])
    do_time_diff = bool(rs.randint(2))
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 10 ** rs.uniform(-2, 4)).astype(dt)
        if rs.randint(2):
            do_time_diff = False                                   # (a float time diff does not keep these bit for bit)
            for v in (np.nan, np.inf, -np.inf, -0.0, 0.0):
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
    for _ in range(3):
        n_cols = int(rs.choice([1, 4, 8, 64, int(rs.randint(1, min(2 * nc + 2, 400)))]))
        cols = [int(c) for c in rs.randint(0, nc, size=n_cols)]
        n4 = -(-n_cols // 4) * 4
        T = int(min(rs.choice([1, 2, 3, 16, 17, 61, 256, int(rs.randint(1, 257))]), max(1, MAX_STEPS // n4)))
        before = int([0, T, min(20, T), int(rs.randint(0, T + 1))][rs.randint(4)])
        K = int(rs.choice([1, 2, 7, int(rs.randint(1, 30))]))
        L = int(rs.choice([1, 1, 2, 3, 9, 64, 65, 300]))
        taps = None if L == 1 and rs.randint(2) else rs.randn(L) / np.sqrt(L)
        reference = [None, 'median'][rs.randint(2)]
        k = rs.randn(K, T, n_cols)
        if rs.randint(3) == 0:
            k[rs.rand(K, T, n_cols) < 0.3] = 0.0
        # the events: none, sparse, clustered on a few rows, or both; the first and the last sample and ties among them
        kind = rs.randint(4)
        n_ev = [0, int(rs.randint(1, 40)), int(rs.randint(20, 400)), int(rs.randint(20, 400))][kind]
        if kind == 2:
            s = rs.randint(0, rows, size=3)[rs.randint(3, size=n_ev)] + rs.randint(0, 3, size=n_ev)
        else:
            s = rs.randint(0, rows, size=n_ev)
        s = np.clip(s, 0, rows - 1)
        if n_ev and rs.randint(2):
            s[rs.randint(n_ev, size=min(n_ev, 4))] = [0, rows - 1, 0, rows - 1][:min(n_ev, 4)]
        amp = (rs.randn(n_ev) * 10 ** rs.uniform(-3, 3)).astype(np.float32)
        for v in (0.0, -0.0, 1e-30, -3e38, 3e38):
            if n_ev and rs.randint(4) == 0:
                amp[rs.randint(n_ev)] = v
        ev = (s, rs.randint(0, K, size=n_ev), amp)
        span = max(1, min(rows, 1500))
        i0 = int([0, max(0, rows - span), int(rs.randint(0, rows))][rs.randint(3)])
        i1 = int(min(rows, i0 + [span, 1, int(rs.randint(1, span + 1))][rs.randint(3)]))
        small = i1 - i0 <= 600
        _env('MTS_RESIDUAL_SLAB_BYTES', [None, 1, 4 * n_cols * 7, 1 << 20][rs.randint(4)] if small else [None, 1 << 20][rs.randint(2)])
        api.RESIDUAL_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
        api.RESIDUAL_OUT_BYTES = [4 * n_cols * 100, 1 << 30][rs.randint(2)]
        t, ref = [1.0] if taps is None else taps, 1 if reference else 0
        what = (dt.name, T, before, n_cols, K, n_ev, i0, i1)
        got = r.residual(*ev, k, i0, i1, channels=cols, before=before, taps=taps, reference=reference)
        want = residual(dec[:, cols], 0, 0, rows, i0, i1, t, ref, before, k, *ev)
        assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes(), ('rows', what)
        # the events of the residual's scores, over a range the oracle can score
        R = int([0, 1, 2, 63, int(rs.randint(0, 256))][rs.randint(5)])
        j1 = int(min(i1, i0 + max(1, 20000 // K)))
        if (j1 - i0 + 2 * R) * K > 60000:
            R = 2
        thr = [np.float32(-3e38), np.float32(0.0), np.float32(10 ** rs.uniform(0, 4))][rs.randint(3)]
        z_row, s_row = 4 * n_cols, 4 * K
        some = max(z_row * (2 * R + T + 70), s_row * (2 * R + 70))
        _env('MTS_TMATCH_SLAB_BYTES', [None, 1, some, 1 << 20][rs.randint(4)] if small else [None, 1 << 20][rs.randint(2)])
        api.TMATCH_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
        api.TMATCH_GUESS_MIN = [1, 16, 4096][rs.randint(3)]
        found = r.match_templates(k, thr, i0, j1, channels=cols, before=before, taps=taps, reference=reference, exclude=R, subtract=ev)
        wev = match_residual(dec[:, cols], 0, 0, rows, i0, j1, t, ref, before, k, thr, R, *ev)
        assert found.sample.tobytes() == wev[0].tobytes(), ('event rows', what, R, found.sample[:6], wev[0][:6])
        assert found.template.tobytes() == wev[1].tobytes(), ('event templates', what, R)
        assert found.score.tobytes() == wev[2].tobytes(), ('event scores', what, R)
    r.close()


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261019))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 5))
    print('fuzz_residual_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
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
    print('fuzz_residual_gpu: %d cases passed' % n, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
