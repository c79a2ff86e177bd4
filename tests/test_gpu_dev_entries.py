"""The device entries of the six reductions (hip.dev_window_stats, dev_rank_hist, dev_decimate, dev_detect, dev_welch, dev_gram) on the
MI355X, on the paths the other GPU tests leave to the bench tools: the `out` DevBuffer passed again, and the results left on the
device (download=False / fetch=False) and copied by hand from the 256-byte aligned offsets.  Every result must have the bytes of the
host entry hip.<op>(0, ...) on the same two chunks."""
import numpy as np
import pytest

from mtscomp_amd import hip
from mtscomp_amd.synth import synth_int16

pytestmark = pytest.mark.gpu

ROWS, NC, COLS = 1000, 8, [5, 0, 5]
N = 2 * ROWS
TAPS = np.linspace(-0.3, 0.5, 9)
N_WIN = -(-N // 512)
CAP = N * len(COLS)                                              # detect: room for an event at every (row, column)

# per op: its own arguments, the keys of a result dict (or None), the flag that leaves the results on the device
OPS = {
    'window_stats': ((0, N, 512, COLS), ('min', 'max', 'sum', 'sumsq'), None),
    'rank_hist': ((0, N, 512, COLS, 0, None, np.zeros((N_WIN, 2, 3), np.uint64),
                   np.repeat(np.array([[8], [-1]], np.int32), 3, axis=1)[None].repeat(N_WIN, axis=0)), ('hist', 'kmin', 'kmax'), 'fetch'),
    'decimate': ((0, N, 4, -(-N // 3), 3, TAPS, np.float32, COLS), None, 'download'),
    'detect': ((0, N, 0, N, TAPS, COLS, [4.0, 5.0, 6.0], 2, 1, 3, 1, CAP), None, 'download'),
    'welch': ((0, 0, (N - 16) // 8 + 1, 16, 8, np.hanning(16), True, np.float32, COLS), None, 'download'),
    'gram': ((0, N, 512, 0, N_WIN, COLS), None, 'download'),
}


@pytest.fixture(scope='module')
def chunks():
    hip.require_device()
    x = synth_int16(0, N, NC, 5)
    bounds = np.array([0, ROWS, N], np.int64)
    zs = hip.compress_chunks(x, bounds, hip.make_flags(), 6)
    data = b''.join(zs)
    offs = np.concatenate(([0], np.cumsum([len(z) for z in zs])))
    cbuf = hip.DevBuffer(len(data) + 256)
    cbuf.upload(np.frombuffer(data + b'\0' * 256, dtype=np.uint8))
    yield data, offs[:-1], np.diff(offs), bounds[:-1], np.diff(bounds), cbuf
    cbuf.free()


def _arrays(op, res):
    """(the arrays the library writes on the device, what it hands back on the host) of a wrapper's result without status and `out`."""
    keys = OPS[op][1]
    if keys:
        return [res[0][k] for k in keys], [res[0]['count']]
    if op == 'detect':
        return list(res[1:] if len(res) == 4 else res[1]), [np.int64(res[0])]
    return list(res), []


def same(got, ref):
    return [(a.dtype, a.shape, a.tobytes()) for a in got] == [(a.dtype, a.shape, a.tobytes()) for a in ref]


@pytest.mark.parametrize('op', list(OPS))
def test_out_again_and_results_left_on_the_device(chunks, op):
    data, offs, lens, row0, rows, cbuf = chunks
    args, _, flag = OPS[op]
    flags = hip.make_flags()
    st, *want = getattr(hip, op)(0, [0, 1], row0, data, offs, lens, rows, NC, np.int16, flags, *args)
    assert st == [0, 0]
    want_dev, want_host = _arrays(op, want)
    assert all(a.size for a in want_dev)
    dev = getattr(hip, 'dev_' + op)
    st, *got, out = dev(cbuf, offs, lens, row0, rows, NC, np.int16, flags, *args)
    assert st == [0, 0] and all(map(same, _arrays(op, got), (want_dev, want_host)))
    st, *got, again = dev(cbuf, offs, lens, row0, rows, NC, np.int16, flags, *args, out=out)
    assert again is out                                           # (large enough: kept)
    assert st == [0, 0] and all(map(same, _arrays(op, got), (want_dev, want_host)))
    if flag:
        out.upload(np.zeros(out.nbytes, np.uint8))
        st, *got, again = dev(cbuf, offs, lens, row0, rows, NC, np.int16, flags, *args, out=out, **{flag: False})
        assert again is out and st == [0, 0]
        if flag == 'download':
            assert all(g is None for g in (got[1:] if op == 'detect' else got))
        assert same(_arrays(op, got)[1], want_host) if op != 'detect' else got[0] == want[0]
        sizes = [CAP * a.dtype.itemsize if op == 'detect' else a.nbytes for a in want_dev]
        at = np.concatenate(([0], np.cumsum([(b + 255) // 256 * 256 for b in sizes])))
        by_hand = [out.download(int(o), a.nbytes, a.dtype).reshape(a.shape) for o, a in zip(at, want_dev)]
        assert same(by_hand, want_dev)
    out.free()
