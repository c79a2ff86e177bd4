"""Randomised parity of Reader.localize on a GPU box: random recordings (all ten item types, channel counts, chunk durations; float
data with NaN, infinities, denormals and zeros of both signs sprinkled in, constant stretches for ties) compressed with
mtscomp_amd.compress and read back with random event lists (any order, repeats, clusters, the first and the last row), snippet
shapes, neighbourhoods, taps, reference, column lists, positions (1 to 4 coordinates, 1-D ones, zeros of both signs, denormals and
huge entries among them), all four amplitude modes, with and without the amplitudes, and cache states.  Each case also draws the
decode pieces (MTS_PIPE_BYTES), the slab bound (MTS_WAVEFORMS_SLAB_BYTES), the gap (MTS_WAVEFORMS_GAP_ROWS), one lane or two on
device 0, WAVEFORMS_CALL_BYTES and WAVEFORMS_OUT_BYTES.
Every comparison is exact: amplitude, weight, moment, best and location byte for byte against tests/localize_oracle.py over the
oracle's decode.

    python tools/fuzz_localize_gpu.py [seed] [seconds]
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
from tests.localize_oracle import MODES, localize, location  # noqa: E402

MAX_SAMPLES = 12000 * 130
MAX_ENTRIES = 1 << 21                                              # of the snippets the oracle builds
DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


def _env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)


def one_case(rs, tmp):
    dt = np.dtype(DTYPES[rs.randint(len(DTYPES))])
    nc = int(rs.choice([1, 2, 3, 17, 64, 65, 70, 130, 257, 600, 1024]))
    rows = int(rs.randint(1, min(12000, MAX_SAMPLES // nc + 1)))
    _env('MTS_PIPE_BYTES', [None, 64 << 10, 300 << 10, 8 << 20][rs.randint(4)])
    _env('MTS_WAVEFORMS_SLAB_BYTES', [None, 1, 40 << 10, 1 << 20][rs.randint(4)])
    _env('MTS_WAVEFORMS_GAP_ROWS', [None, 0, 1, 100, -1][rs.randint(5)])
    api.WAVEFORMS_CALL_BYTES = [1, 1 << 16, 1 << 30][rs.randint(3)]
    api.WAVEFORMS_OUT_BYTES = [1, 1 << 12, 1 << 30][rs.randint(3)]
    do_time_diff = bool(rs.randint(2))
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 10 ** rs.uniform(-2, 4)).astype(dt)
        if rs.randint(2):
            do_time_diff = False                                   # (a float time diff does not keep these bit for bit)
            for v in (np.nan, np.inf, -np.inf, -0.0, 1e-42, -3e-39, 3e38, -3e38):
                x[rs.randint(rows, size=2), rs.randint(nc, size=2)] = v
            if rs.randint(2):
                a = int(rs.randint(rows))
                x[a:a + int(rs.randint(1, 40))] = np.nan           # whole snippets of NaN
            if rs.randint(2):
                a = int(rs.randint(rows))
                x[a:a + int(rs.randint(1, 200))] = float(rs.randint(-2, 3))     # constant rows: ties in every column and between columns
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
        cols = [int(c) for c in rs.randint(0, nc, size=rs.randint(1, min(2 * nc + 2, 1025)))]
        L = int(rs.choice([1, 1, 2, 3, 9, 64, 65, 300]))
        taps = None if L == 1 and rs.randint(2) else rs.randn(L) / np.sqrt(L)
        reference = [None, 'median'][rs.randint(2)]
        before, after = [(20, 41), (0, 1), (1, 0), (5, 0), (0, 7), (3, 3), (2048, 2048), (int(rs.randint(0, 200)), int(rs.randint(1, 200)))][rs.randint(8)]
        T = before + after
        k = [None, 0, 1, 8, 32, 63, 64, 127, 128, int(rs.randint(0, 512))][rs.randint(10)]
        W = len(cols) if k is None else 2 * k + 1
        n_ev = int(rs.randint(0, max(2, min(600, MAX_ENTRIES // (T * W)))))
        kind = rs.randint(3)
        if kind == 0:
            sample = rs.randint(0, rows, n_ev)
        elif kind == 1:                                            # two clusters far apart: chunks between them are not read
            sample = np.concatenate((rs.randint(0, max(1, rows // 10), n_ev // 2), rs.randint(rows - max(1, rows // 10), rows, n_ev - n_ev // 2)))
            sample = sample[rs.permutation(n_ev)]
        else:                                                      # repeats and the two ends
            sample = rs.choice(np.array([0, rows - 1, rows // 2, int(rs.randint(rows))]), n_ev)
        channel = np.asarray(cols)[rs.randint(0, len(cols), n_ev)]
        D = int(rs.randint(1, 5))
        pos = (rs.randn(len(cols), D) * 10 ** rs.uniform(-3, 4)).astype(np.float32)
        for v in (0.0, -0.0, 1e-42, 3e38, -3e38, -2.0 ** -126):
            if rs.randint(2):
                pos[rs.randint(len(cols)), rs.randint(D)] = v
        flat = D == 1 and bool(rs.randint(2))
        mode = sorted(MODES)[rs.randint(4)]
        with_amp = bool(rs.randint(4))
        got = r.localize(sample, pos[:, 0] if flat else pos, channel, before=before, after=after, neighbours=k, channels=cols, taps=taps,
                         reference=reference, amplitude=mode, amplitudes=with_amp)
        col0 = np.zeros(n_ev, np.int64) if k is None else np.array([cols.index(c) for c in channel], np.int64) - k
        amp, weight, moment, best = localize(dec[:, cols], 0, 0, rows, [1.0] if taps is None else taps, 1 if reference else 0, sample, col0,
                                             before, after, W, MODES[mode], pos)
        loc = location(moment, weight)
        chan = np.where(best >= 0, np.asarray(cols)[np.where(best >= 0, col0 + best, 0)], -1)
        want = dict(amplitude=amp if with_amp else None, weight=weight, moment=moment[:, 0] if flat else moment, best=best,
                    location=loc[:, 0] if flat else loc, channel=chan)
        for name, w in want.items():
            g = got[name]
            if w is None:
                assert g is None, name
                continue
            assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (name, mode, W, T, D, np.argwhere(np.atleast_1d(g != w) & ~(np.isnan(g) & np.isnan(w)))[:4].tolist())
        assert got.positions.tobytes() == pos.tobytes() and np.array_equal(got.position, col0) and got.mode == mode, 'bunch'
    r.close()


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else int(os.environ.get('MTS_FUZZ_SEED', 20261020))
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else float(os.environ.get('MTS_FUZZ_SECONDS', 5))
    print('fuzz_localize_gpu: seed %d, %.0f s' % (seed, seconds), flush=True)
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
    print('fuzz_localize_gpu: %d cases passed' % n, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
