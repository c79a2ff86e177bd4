"""bench.py's own options: --steps / --full / --dump-outputs.  On CPU: the flags and the dump (bench.dump_outputs) on stand-ins for
the device buffers; under -m gpu: a small plain run whose dumped outputs are checked against the generator and the oracle."""
import json
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

import bench
from mtscomp_amd.synth import synth_int16

ROOT = Path(__file__).resolve().parent.parent
CONTRACT_KEYS = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


class HostStandIn:
    """What dump_outputs needs of a hip.DevBuffer (download), over a host array."""

    def __init__(self, arr):
        self.a = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        self.nbytes = self.a.size

    def download(self, offset=0, nbytes=None, dtype=np.uint8):
        nbytes = self.nbytes - offset if nbytes is None else int(nbytes)
        assert 0 <= offset and offset + nbytes <= self.nbytes
        return self.a[offset:offset + nbytes].copy().view(dtype)


class ZerosStandIn:
    """A device buffer of `nbytes` zero bytes that is never held whole on the host."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)

    def download(self, offset=0, nbytes=None, dtype=np.uint8):
        nbytes = self.nbytes - offset if nbytes is None else int(nbytes)
        assert 0 <= offset and offset + nbytes <= self.nbytes
        return np.zeros(nbytes, dtype=np.uint8).view(dtype)


def test_flags():
    a = bench.parse_args([])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 1, False, None)
    a = bench.parse_args(['--steps', '7', '--warmup', '0', '--full', '--dump-outputs', 'somewhere'])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 0, True, 'somewhere')
    for bad in (['--steps', '0'], ['--warmup', '-1']):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def _stand_in_outputs(n, rate, nc):
    x = synth_int16(0, n * rate, nc, 3)
    streams = [zlib.compress(x[k * rate:(k + 1) * rate].tobytes(), 6) for k in range(n)]
    streams[1] = streams[1][:40]                                  # one stream shorter than the head and the sample
    bound = max(map(len, streams)) + 256
    slots = np.arange(n, dtype=np.int64) * bound
    cbuf = np.zeros(n * bound, dtype=np.uint8)
    for k, z in enumerate(streams):
        cbuf[slots[k]:slots[k] + len(z)] = np.frombuffer(z, dtype=np.uint8)
    sizes = np.array([len(z) for z in streams], dtype=np.int64)
    status = np.zeros(n, dtype=np.int32)
    status[2] = -1
    return x, streams, HostStandIn(cbuf), slots, sizes, HostStandIn(x), status


def test_dump_outputs_are_the_outputs(tmp_path):
    n, rate, nc = 5, 3000, 24
    x, streams, cbuf, slots, sizes, back, status = _stand_in_outputs(n, rate, nc)
    names = bench.dump_outputs(tmp_path / 'a', cbuf, slots, sizes, back, status, n, rate, nc)
    got = {name: np.load(tmp_path / 'a' / (name + '.npy')) for name in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert list(got['compressed_sizes']) == [len(z) for z in streams]
    assert list(got['chunk_status']) == [0, 0, -1, 0, 0]
    H, T = got['compressed_head'].shape[1], got['compressed_tail'].shape[1]
    frac = np.sort(np.random.RandomState(bench.DUMP_SEED).random_sample(got['compressed_sample'].shape[1]))
    for k, z in enumerate(streams):
        zb = np.frombuffer(z, dtype=np.uint8).astype(np.float32)
        head = np.full(H, -1, dtype=np.float32)
        head[:min(H, len(z))] = zb[:H]
        tail = np.full(T, -1, dtype=np.float32)
        tail[T - min(T, len(z)):] = zb[len(z) - min(T, len(z)):]
        assert np.array_equal(got['compressed_head'][k], head) and np.array_equal(got['compressed_tail'][k], tail)
        assert np.array_equal(got['compressed_sample'][k], zb[np.minimum((frac * len(z)).astype(np.int64), len(z) - 1)])
    rows = got['decompressed_rows'].astype(np.int64)
    assert np.array_equal(rows, np.arange(n * rate))                   # (small enough to be dumped whole)
    assert np.array_equal(got['decompressed_sample'], x[rows].astype(np.float32))
    # the same outputs give the same files
    bench.dump_outputs(tmp_path / 'b', cbuf, slots, sizes, back, status, n, rate, nc)
    assert all((tmp_path / 'a' / (f + '.npy')).read_bytes() == (tmp_path / 'b' / (f + '.npy')).read_bytes() for f in names)


@pytest.mark.parametrize('n,rate,nc', [(60, 30000, 385), (300, 7500, 1024), (450, 30000, 385)], ids=['headline', 'stress', 'config3_rank'])
def test_dump_outputs_stay_under_64_mb(tmp_path, n, rate, nc):
    """The default workloads' outputs (GBs) come out as a seeded sample of at most 64 MB, rows drawn from the whole recording."""
    bound = 1 << 16
    sizes = np.full(n, 50000, dtype=np.int64)
    names = bench.dump_outputs(tmp_path, ZerosStandIn(n * bound), np.arange(n, dtype=np.int64) * bound, sizes,
                               ZerosStandIn(n * rate * nc * 2), np.zeros(n, dtype=np.int32), n, rate, nc)
    assert sum((tmp_path / (f + '.npy')).stat().st_size for f in names) <= 64 << 20
    rows = np.load(tmp_path / 'decompressed_rows.npy')
    assert rows.size < n * rate and rows.min() < rate and rows.max() >= (n - 1) * rate and np.all(np.diff(rows) > 0)


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(tmp_path):
    """A plain run: the contract's keys, exactly --steps timed steps, none of --full's checks or measurements, and the dumped
    outputs equal to the generator's rows and the reference's bytes (numpy + zlib level 6, the oracle)."""
    from oracle import oracle as O
    out = tmp_path / 'outputs'
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, str(ROOT / 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--seconds', '3',
                        '--dump-outputs', str(out)], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert all(k in line for k in CONTRACT_KEYS) and line['value'] > 0 and line['ms_per_step'] > 0
    assert (line['steps'], line['warmup'], line['full'], line['byte_identical_chunk0']) == (2, 1, False, None)
    assert not any(k in line for k in ('cpu_baseline', 'extras', 'level_curve'))
    assert abs(line['ms_per_step'] - 3 * 30000 * 385 * 2 / (line['value'] * 1e9) * 1e3) < 1e-6 * line['ms_per_step']
    assert sorted(line['dumped_outputs']) == sorted(p.stem for p in out.glob('*.npy'))
    x = synth_int16(0, 3 * 30000, 385, 0)
    rows = np.load(out / 'decompressed_rows.npy').astype(np.int64)
    assert np.array_equal(np.load(out / 'decompressed_sample.npy'), x[rows].astype(np.float32))
    assert not np.load(out / 'chunk_status.npy').any()
    sizes, head, tail = (np.load(out / (f + '.npy')) for f in ('compressed_sizes', 'compressed_head', 'compressed_tail'))
    for k in range(3):
        want = np.frombuffer(O.ref_compress_chunk(x[k * 30000:(k + 1) * 30000]), dtype=np.uint8)
        assert sizes[k] == want.size
        assert np.array_equal(head[k], want[:head.shape[1]]) and np.array_equal(tail[k], want[-tail.shape[1]:])
