"""The call plan of the six device reductions, pinned: which codec method Reader.window_stats / quantile / mad / decimate / detect /
welch / cov call, on which lane, for which chunks, with which arguments, in which order.  The numpy stand-ins of tests/*_oracle.py sit
behind one Reader; a thin subclass logs every call.  Calls of one run_lanes batch run on threads: a batch is sorted by lane (a lane's own
calls keep their order), the batches stay in sequence.  EXPECTED was written by the code as it stood before the planner and the lane
drivers of the Reader were shared (python -m tests.test_reduce_plan prints it): per case the (lane: keys) of every call in the clear,
batches separated by '|', and a sha256 over the canonical repr of the whole log."""
import hashlib

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.decimate_oracle import DecimateOracleCodec
from tests.detect_oracle import DetectOracleCodec
from tests.gram_oracle import GramOracleCodec
from tests.select_oracle import SelectOracleCodec
from tests.stats_oracle import StatsOracleCodec
from tests.welch_oracle import WelchOracleCodec

METHODS = ('window_stats', 'rank_hist', 'decimate', 'detect', 'welch', 'gram')
START, STOP, WINDOW, COLS = 700, 8500, 1300, [5, 0, 3]          # off chunk (1000 rows) and window boundaries
TAPS = np.linspace(-0.3, 0.5, 9)


def _canon(v):
    """An argument as something whose repr does not depend on the numpy at hand."""
    if v is None or isinstance(v, (bool, str)):
        return v
    if isinstance(v, np.dtype) or isinstance(v, type):
        return str(np.dtype(v))
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    a = np.ascontiguousarray(v)
    return ('array', str(a.dtype), a.shape, hashlib.sha256(a.tobytes()).hexdigest())


class PlanCodec(GramOracleCodec, SelectOracleCodec, StatsOracleCodec, DecimateOracleCodec, DetectOracleCodec, WelchOracleCodec):
    """The six stand-ins behind one Reader, every call logged."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.log, self._batch = [], None

    def run_lanes(self, fn, n):
        self._batch = []
        try:
            super().run_lanes(fn, n)
        finally:
            batch, self._batch = self._batch, None
            self.log.append(sorted(batch, key=lambda c: c[1]))

    def _logged(self, name, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, *args, lane=None):
        sent = hashlib.sha256(b''.join(bytes(memoryview(cdata)[o:o + n]) for o, n in zip(offs, lens))).hexdigest()
        entry = (name, lane, self.cache_lane[cache_id] if cache_id else None) + \
            tuple(tuple(int(x) for x in seq) for seq in (keys, row0, offs, lens, n_rows)) + \
            (sent, int(n_channels), str(np.dtype(dtype)), int(flags)) + tuple(_canon(a) for a in args)
        if self._batch is None:                                   # (a call outside run_lanes is a batch of its own)
            self.log.append([entry])
        else:
            self._batch.append(entry)
        return getattr(super(), name)(cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, *args, lane=lane)


for _name in METHODS:
    setattr(PlanCodec, _name, (lambda name: lambda self, *a, **kw: self._logged(name, *a, **kw))(_name))


OPS = {
    'window_stats': lambda r: r.window_stats(WINDOW, START, STOP, COLS),
    'quantile': lambda r: r.quantile([0.1, 0.5], START, STOP, COLS, window=WINDOW),
    'mad': lambda r: r.mad(START, STOP, COLS, window=WINDOW),
    'decimate': lambda r: r.decimate(3, START, STOP, COLS, taps=TAPS),
    'detect': lambda r: r.detect([4.0, 5.0, 6.0], START, STOP, COLS, taps=TAPS, sign='both', reference='median', exclude=3, spread=1),
    'welch': lambda r: r.welch(64, START, STOP, COLS),
    'cov': lambda r: r.cov(START, STOP, COLS, window=WINDOW),
}
# per op: the module attribute that cuts by compressed bytes, and (attribute, value) of a results slab small enough to cut first:
# two chunks' tiles of window_stats (3 tiles x 3 columns x 32 bytes each), two windows' histograms, three groups' Gram matrices and sums
BYTES = {'window_stats': 'WINDOW_STATS_CALL_BYTES', 'quantile': 'QUANTILE_CALL_BYTES', 'mad': 'QUANTILE_CALL_BYTES',
         'decimate': 'DECIMATE_CALL_BYTES', 'detect': 'DETECT_CALL_BYTES', 'welch': 'WELCH_CALL_BYTES', 'cov': 'GRAM_CALL_BYTES'}
SLABS = {'window_stats': ('WINDOW_STATS_SLAB_BYTES', 2 * 3 * 3 * 32), 'quantile': ('QUANTILE_SLAB_BYTES', 2 * 2 * (4 * 256 + 16) * 3),
         'cov': ('GRAM_SLAB_BYTES', 3 * 8 * (3 * 3 + 3))}
CASES = [(op, lanes, cut) for op in OPS for lanes in (1, 2, 3) for cut in ('default', 'bytes', 'slab', 'resident')
         if (cut != 'slab' or op in SLABS) and (cut == 'default' or op != 'mad')]


def _run(tmp, monkeypatch, op, lanes, cut):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp / '.mtscomp')
    api.set_codec(None)
    monkeypatch.setattr(hip, 'GRAM_GROUP_ROWS', 1 << 10)
    monkeypatch.setattr(hip, 'WELCH_GROUP_ROWS', 1 << 11)
    monkeypatch.setattr(api, 'DETECT_GUESS_MIN', 7)               # (the first event buffer of a detect call is short: one more call)
    monkeypatch.setattr(api, 'DETECT_GUESS_SAMPLES', 1 << 40)
    if cut == 'bytes':
        monkeypatch.setattr(api, BYTES[op], 1)
    if cut == 'slab':
        monkeypatch.setattr(api, *SLABS[op])
    x = synth_int16(0, 9000, 8, 3)
    x.tofile(tmp / 'data.bin')
    codec = PlanCodec(n_lanes=lanes, capacity_chunks=8)
    mtscomp_amd.compress(tmp / 'data.bin', tmp / 'data.cbin', tmp / 'data.ch', sample_rate=1000., n_channels=8, dtype=x.dtype,
                         codec=codec, check_after_compress=False)
    r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', codec=codec, check_after_decompress=False)
    assert r.chunk_bounds == list(range(0, 9001, 1000))
    if cut == 'resident':                                         # chunks 2, 4 and 5 (and what was read ahead) lie in their owner lanes' caches
        r[2100:2200]
        r[4900:5100]
        codec.log.clear()
    OPS[op](r)
    r.close()
    plan = '|'.join(' '.join('%d:%s' % (c[1], ','.join(map(str, c[3]))) for c in batch) for batch in codec.log)
    return plan, hashlib.sha256(repr(codec.log).encode()).hexdigest(), codec.log


EXPECTED = {
    'window_stats-1-default': ('0:0,1,2,3,4,5,6,7,8',
        '39343b3b2b89a09cf79f39b11b2fd8e208a9eee2e9a463243be1b2dec96f749d'),
    'window_stats-1-bytes': ('0:0|0:1|0:2|0:3|0:4|0:5|0:6|0:7|0:8',
        'fab04ac86b45152d2b596937ba63451d8a443ff7f75e1b9ec9aae2ca0e361e5f'),
    'window_stats-1-slab': ('0:0,1|0:2,3|0:4,5|0:6,7|0:8',
        'b69dea31cc8864c2192f2ef8621eb5e645aecd0ddc5f3af5a31347c28b1257de'),
    'window_stats-1-resident': ('0:0,1,2,3,4,5,6,7,8',
        'ccdeb21d9aadbe266a6ddc74efde0b432c6c954480aee44271189c67522690be'),
    'window_stats-2-default': ('0:0,2,4,6,8 1:1,3,5,7',
        'f7f894772279e28e799dd192bb8b76ed059b3004430fd4bbb17f12f20a2ec27a'),
    'window_stats-2-bytes': ('0:0|1:1|0:2|1:3|0:4|1:5|0:6|1:7|0:8',
        '446a633a9ad08487511e8069aa77768ae48377d69305ddba2f4e2f34f2dc55df'),
    'window_stats-2-slab': ('0:0 1:1|0:2 1:3|0:4 1:5|0:6 1:7|0:8',
        'aab9918b0f5ec47a302957764909090aa1664d87649ddd81d51b6afb45e35c46'),
    'window_stats-2-resident': ('0:0,2,4,6,8 1:1,3,5,7',
        '4c637a82384ef21a2f8b02550502afa41ba31d794c167a167dc7d21a72b1de8c'),
    'window_stats-3-default': ('0:0,3,6 1:1,4,7 2:2,5,8',
        'd674b64eab9c1d8d904fc756f34761fa53c63b04ca2a414210f91d9485305d99'),
    'window_stats-3-bytes': ('0:0|1:1|2:2|0:3|1:4|2:5|0:6|1:7|2:8',
        '25718a0ac57b198c3fc86c5b62dffc3299ecd2ffd2e0ccd46f14c36df14af59f'),
    'window_stats-3-slab': ('0:0 1:1|0:3 2:2|1:4 2:5|0:6 1:7|2:8',
        '45582c321c17b494a491e76def43109a6ad68ff0b868392b0f303a6af1d3e6da'),
    'window_stats-3-resident': ('0:0,3,6 1:1,4,7 2:2,5,8',
        'e719689d61468cd7f471e1f66055bced167a8bb3fdb45db0d3af0be6e4bd391c'),
    'quantile-1-default': ('0:0,1,2,3,4,5,6,7,8|0:0,1,2,3,4,5,6,7,8|0:0,1,2,3,4,5,6,7,8|0:0,1,2,3,4,5,6,7,8',
        'e2f8dd3324aa5e24207a53e30c73e7a73d4f508dc98bce92ed35a70608599250'),
    'quantile-1-bytes': ('0:0|0:1|0:2|0:3|0:4|0:5|0:6|0:7|0:8|0:0|0:1|0:2|0:3|0:4|0:5|0:6|0:7|0:8|0:0|0:1|0:2|0:3|0:4|0:5|0:6|0:7|0:8|0:0|0:1|0:2|0:3|0:4|0:5|0:6|0:7|0:8',
        '84e20a9624c8e0a7a20b035083c7a91c9191c45e76433f4481f24c160e55ca5e'),
    'quantile-1-slab': ('0:0,1,2,3|0:0,1,2,3|0:0,1,2,3|0:0,1,2,3|0:3,4,5|0:3,4,5|0:3,4,5|0:3,4,5|0:5,6,7,8|0:5,6,7,8|0:5,6,7,8|0:5,6,7,8',
        '31cb2301ee22debfc2034f2226614abeb5170d3f276a80feb47fe4f065a148b7'),
    'quantile-1-resident': ('0:0,1,2,3,4,5,6,7,8|0:0,1,2,3,4,5,6,7,8|0:0,1,2,3,4,5,6,7,8|0:0,1,2,3,4,5,6,7,8',
        'a22bdc2bfe4e8e3d02fe5d1f3ffae526970ebe897d24519b7288ee523e78a15d'),
    'quantile-2-default': ('0:0,2,4,6,8 1:1,3,5,7|0:0,2,4,6,8 1:1,3,5,7|0:0,2,4,6,8 1:1,3,5,7|0:0,2,4,6,8 1:1,3,5,7',
        '63b9d340cbc2a4bc6db5229ade50cedfcc96162b918ea579162a48117d0f075b'),
    'quantile-2-bytes': ('0:0|1:1|0:2|1:3|0:4|1:5|0:6|1:7|0:8|0:0|1:1|0:2|1:3|0:4|1:5|0:6|1:7|0:8|0:0|1:1|0:2|1:3|0:4|1:5|0:6|1:7|0:8|0:0|1:1|0:2|1:3|0:4|1:5|0:6|1:7|0:8',
        '18dd3ddd7579153f86cfc945b93410858ebb3d9887292e2ead30efea22ae8f00'),
    'quantile-2-slab': ('0:0,2 1:1,3|0:0,2 1:1,3|0:0,2 1:1,3|0:0,2 1:1,3|0:4 1:3,5|0:4 1:3,5|0:4 1:3,5|0:4 1:3,5|0:6,8 1:5,7|0:6,8 1:5,7|0:6,8 1:5,7|0:6,8 1:5,7',
        '2d37caefa8111438597ced63873cb8f90d5ae1c1d9d5e5ca0ba23431997d4459'),
    'quantile-2-resident': ('0:0,2,4,6,8 1:1,3,5,7|0:0,2,4,6,8 1:1,3,5,7|0:0,2,4,6,8 1:1,3,5,7|0:0,2,4,6,8 1:1,3,5,7',
        'b5d90c570be045891779dae8ad79d7fae17f5a05724f533a7a001cc920f5fbff'),
    'quantile-3-default': ('0:0,3,6 1:1,4,7 2:2,5,8|0:0,3,6 1:1,4,7 2:2,5,8|0:0,3,6 1:1,4,7 2:2,5,8|0:0,3,6 1:1,4,7 2:2,5,8',
        '743ef0103f6307f2d7e2d580c08a7c643dc713d2117ca85a1f40ad1da2bfb181'),
    'quantile-3-bytes': ('0:0|1:1|2:2|0:3|1:4|2:5|0:6|1:7|2:8|0:0|1:1|2:2|0:3|1:4|2:5|0:6|1:7|2:8|0:0|1:1|2:2|0:3|1:4|2:5|0:6|1:7|2:8|0:0|1:1|2:2|0:3|1:4|2:5|0:6|1:7|2:8',
        '22bdec15c3d055cb27a06812985ae731acde91b0f619756f710527a9b67a3863'),
    'quantile-3-slab': ('0:0,3 1:1 2:2|0:0,3 1:1 2:2|0:0,3 1:1 2:2|0:0,3 1:1 2:2|0:3 1:4 2:5|0:3 1:4 2:5|0:3 1:4 2:5|0:3 1:4 2:5|0:6 1:7 2:5,8|0:6 1:7 2:5,8|0:6 1:7 2:5,8|0:6 1:7 2:5,8',
        '04ada4f5ed1238ed3e5d6d3761b50a02209617b3feee6b70d107144b84d22e24'),
    'quantile-3-resident': ('0:0,3,6 1:1,4,7 2:2,5,8|0:0,3,6 1:1,4,7 2:2,5,8|0:0,3,6 1:1,4,7 2:2,5,8|0:0,3,6 1:1,4,7 2:2,5,8',
        '46ec52d3479462261b567ac220bcfefe8f17223000aeea5b45845eb46968b857'),
    'mad-1-default': ('0:0,1,2,3,4,5,6,7,8|0:0,1,2,3,4,5,6,7,8|0:0,1,2,3,4,5,6,7,8|0:0,1,2,3,4,5,6,7,8|0:0,1,2,3,4,5,6,7,8',
        'd8a526dac6f56f3c0934cbe4bd166b7a0f35d6269ad792139ee8ddf03d2046ac'),
    'mad-2-default': ('0:0,2,4,6,8 1:1,3,5,7|0:0,2,4,6,8 1:1,3,5,7|0:0,2,4,6,8 1:1,3,5,7|0:0,2,4,6,8 1:1,3,5,7|0:0,2,4,6,8 1:1,3,5,7',
        'c7383a6178065fca01ab0baa41cd08e80193a2661fff21123feaf621c646b935'),
    'mad-3-default': ('0:0,3,6 1:1,4,7 2:2,5,8|0:0,3,6 1:1,4,7 2:2,5,8|0:0,3,6 1:1,4,7 2:2,5,8|0:0,3,6 1:1,4,7 2:2,5,8|0:0,3,6 1:1,4,7 2:2,5,8',
        '33bb9f926da13578253657c3ffcde347d3f3738f86d42964aba31bd854aa6af3'),
    'decimate-1-default': ('0:0,1,2,3,4,5,6,7,8',
        'c6b8f2c87bcc5f0e518e711190613c8045ddccc3f32d2365d3d2b21063c0ce1f'),
    'decimate-1-bytes': ('0:0|0:0,1|0:1,2|0:2,3|0:3,4|0:4,5|0:5,6|0:6,7|0:7,8',
        'f89f21fa58c7fa996525a9e6c06ef1dc76aeff18e6fb4237b61294a626c33221'),
    'decimate-1-resident': ('0:0,1,2,3,4,5,6,7,8',
        '41958948229aebbe997f8a1e6c2f261122c3d1163d550f2ffea8e66a922a1020'),
    'decimate-2-default': ('0:0,1,2,3,4 1:4,5,6,7,8',
        '7e4864565e6944aa84f77f1b2a15247d2622a45584f644ebd9064a45e89eed04'),
    'decimate-2-bytes': ('0:0 1:0|0:0,1 1:1|0:1,2 1:2|0:2,3 1:3|0:3,4 1:4|0:4,5 1:5|0:5,6 1:6|0:6,7 1:7|0:7,8 1:8',
        'baef9ee0130cc1e7e6a1c3c9dc1e5424ecb0e8f3d3d121f745dfdd6f05be49b7'),
    'decimate-2-resident': ('0:0,1,2,3,4 1:4,5,6,7,8',
        'a33ebc78181952b9306183b1297d407e0808ba062961ba1bf3e8148cd10baf09'),
    'decimate-3-default': ('0:0,1,2,3 1:3,4,5 2:5,6,7,8',
        '92db4f2f6231c402fd30f2a07ae6838a1545cbd7e583d06e9f4567abd5dcc627'),
    'decimate-3-bytes': ('0:0 1:0 2:0|0:0,1 1:1 2:1|0:1,2 1:2 2:2|0:2,3 1:3 2:3|0:3,4 1:4 2:4|0:4,5 1:5 2:5|0:5,6 1:6 2:6|0:6,7 1:7 2:7|0:7,8 1:8 2:8',
        '09f9ffc82c6c42d30bcc9a135515b319f64bc664b306fb9637c321e80cc1685a'),
    'decimate-3-resident': ('0:0,1,2,3 1:3,4,5 2:5,6,7,8',
        '824bad53809e2093607e50c12f4f0e6c01b241ffbc72a64ac939665b91344250'),
    'detect-1-default': ('0:0,1,2,3,4,5,6,7,8 0:0,1,2,3,4,5,6,7,8',
        '3536d8de766770f86c23c539626a28d7f2cfaad55f100647ebd32a29f5d62264'),
    'detect-1-bytes': ('0:0,1 0:0,1|0:0,1,2 0:0,1,2|0:1,2,3 0:1,2,3|0:2,3,4 0:2,3,4|0:3,4,5 0:3,4,5|0:4,5,6 0:4,5,6|0:5,6,7 0:5,6,7|0:6,7,8 0:6,7,8|0:7,8 0:7,8',
        '0da72dde2d17dea0dbfb4f6fe9900a0baa98e741d2ea864947a23ac2eab981ee'),
    'detect-1-resident': ('0:0,1,2,3,4,5,6,7,8 0:0,1,2,3,4,5,6,7,8',
        '5617aea300b60a98d846b0bac4ac36784df24a858df3f459311bc3785dbd6e74'),
    'detect-2-default': ('0:0,1,2,3,4 0:0,1,2,3,4 1:4,5,6,7,8 1:4,5,6,7,8',
        '3997493010e7a958400a80623c6f2e8c86e68cf8d44216a243d6c238192a8ff1'),
    'detect-2-bytes': ('0:0 0:0 1:0,1 1:0,1|0:0,1 0:0,1 1:1,2 1:1,2|0:1,2 0:1,2 1:2,3 1:2,3|0:2,3 0:2,3 1:3,4 1:3,4|0:3,4 0:3,4 1:4,5 1:4,5|0:4,5 0:4,5 1:5,6 1:5,6|0:5,6 0:5,6 1:6,7 1:6,7|0:6,7 0:6,7 1:7,8 1:7,8|0:7,8 0:7,8 1:8 1:8',
        'e67d271c3abeb616ff33f932bed0b924a19a49b6096ff95478e110c71070d1e2'),
    'detect-2-resident': ('0:0,1,2,3,4 0:0,1,2,3,4 1:4,5,6,7,8 1:4,5,6,7,8',
        '63f43dcd2c0c1ae55ecf9138de0f57de22e30329ecede9bd9e655c9c7a82bda1'),
    'detect-3-default': ('0:0,1,2,3 0:0,1,2,3 1:3,4,5 1:3,4,5 2:5,6,7,8 2:5,6,7,8',
        'c01abd274e94b3873acd064c324697eb7ef3e4156d1271e09187ebca8d153278'),
    'detect-3-bytes': ('0:0 0:0 1:0 1:0 2:0,1 2:0,1|0:0,1 0:0,1 1:1 1:1 2:1,2 2:1,2|0:1,2 0:1,2 1:2 1:2 2:2,3 2:2,3|0:2,3 0:2,3 1:3 1:3 2:3,4 2:3,4|0:3,4 0:3,4 1:4 1:4 2:4,5 2:4,5|0:4,5 0:4,5 1:5 1:5 2:5,6 2:5,6|0:5,6 0:5,6 1:6 1:6 2:6,7 2:6,7|0:6,7 0:6,7 1:7 1:7 2:7,8 2:7,8|0:7,8 0:7,8 1:8 1:8 2:8 2:8',
        '41e9d62908926504b7b66641508d77e377af0884fb8a93599838c8af5d3dc11d'),
    'detect-3-resident': ('0:0,1,2,3 0:0,1,2,3 1:3,4,5 1:3,4,5 2:5,6,7,8 2:5,6,7,8',
        'e74525dcb6fbbd8b5c4863d131954fba6d26e0b984b3116cd4e72b0f66482178'),
    'welch-1-default': ('0:0,1,2,3,4,5,6,7,8',
        '5712d7268563d40fcfa18a32cbb5ebed6f9a9fbc57cb11036fe7e0b869bcebca'),
    'welch-1-bytes': ('0:0,1,2|0:2,3,4|0:4,5,6|0:6,7,8',
        '4a3a5812a2e022a8f28de460b81aa77ae4c30784d7e6717cb0110961c966bdc8'),
    'welch-1-resident': ('0:0,1,2,3,4,5,6,7,8',
        '746c3200850a2ec2b2e1697224a884ba4f3adf12cd21df3901221d9988308f27'),
    'welch-2-default': ('0:0,1,2,3,4 1:4,5,6,7,8',
        'f0e9429928390cfec6ae5aec0ff860cb7e89d5edd3552709d998e1aff97721d4'),
    'welch-2-bytes': ('0:0,1,2|0:2,3,4|0:4,5,6|0:6,7,8',
        '4a3a5812a2e022a8f28de460b81aa77ae4c30784d7e6717cb0110961c966bdc8'),
    'welch-2-resident': ('0:0,1,2,3,4 1:4,5,6,7,8',
        'cc0e9d37820a694f2cc57c38611c7586743dd9598e7736b496f702a0746a2e9e'),
    'welch-3-default': ('0:0,1,2 1:2,3,4 2:4,5,6,7,8',
        '62377040a7e21795e8f9dd04118b9bd0a17deb8c1b91f51e7e54fabff14b3789'),
    'welch-3-bytes': ('0:0,1,2|0:2,3,4|0:4,5,6|0:6,7,8',
        '4a3a5812a2e022a8f28de460b81aa77ae4c30784d7e6717cb0110961c966bdc8'),
    'welch-3-resident': ('0:0,1,2 1:2,3,4 2:4,5,6,7,8',
        '9f484727f1ab686f61bb6b066d43abcd1cf9c7e7e6db98395d6f9bbdb3ca084e'),
    'cov-1-default': ('0:0,1,2,3,4,5,6,7,8',
        '0be09ca505f4019d1b2b17e86c8c2918d6ee388d40dc52e58eb0e91a65b13805'),
    'cov-1-bytes': ('0:0,1|0:1|0:2,3|0:3|0:3,4|0:4|0:4,5|0:5|0:5,6|0:6,7|0:7,8|0:8',
        '91118c1be5a0880f9ca48f24974e6d1b2da40dec03ca869b42d12e5f0fe23292'),
    'cov-1-slab': ('0:0,1,2,3|0:3,4|0:4,5,6|0:6,7,8',
        '522d0d578ff270faccafe08b21af683cba8b3324a479266d0001b3b1017578a5'),
    'cov-1-resident': ('0:0,1,2,3,4,5,6,7,8',
        '823d9cbbff9bca46d8b0f7ec56b2ec6cd3587e19c480ab00bff0ebbf814b8d74'),
    'cov-2-default': ('0:0,1,2,3,4 1:4,5,6,7,8',
        'cd332438a033336eb3b715a5c45be9b943cd1c23356b82df9b397fb7838d9c9d'),
    'cov-2-bytes': ('0:0,1|0:1|0:2,3|0:3|0:3,4|0:4|0:4,5|0:5|0:5,6|0:6,7|0:7,8|0:8',
        '91118c1be5a0880f9ca48f24974e6d1b2da40dec03ca869b42d12e5f0fe23292'),
    'cov-2-slab': ('0:0,1 1:1,2,3|0:3 1:3,4|0:4,5 1:5,6|0:6,7 1:7,8',
        '5a2591e4764fbb0e7987fa699b484bb91b2c814c18952ed6ba13829b608d8686'),
    'cov-2-resident': ('0:0,1,2,3,4 1:4,5,6,7,8',
        'd64612d4226123bf779de9b48dcc4d11b40f519ffc27237a259cdef614998cc9'),
    'cov-3-default': ('0:0,1,2,3 1:3,4,5 2:5,6,7,8',
        '79c345cf1df5114a7424555a0098949f71d9862b969284f71cb0fa1819d1feab'),
    'cov-3-bytes': ('0:0,1|0:1|0:2,3|0:3|0:3,4|0:4|0:4,5|0:5|0:5,6|0:6,7|0:7,8|0:8',
        '91118c1be5a0880f9ca48f24974e6d1b2da40dec03ca869b42d12e5f0fe23292'),
    'cov-3-slab': ('0:0,1 1:1 2:2,3|0:3 1:3,4 2:4|0:4,5 1:5 2:5,6|0:6,7 1:7,8 2:8',
        'f04ee59bc0f3db0564a57abf30691035669c46edb6f4849e3e0ff147ac3792ee'),
    'cov-3-resident': ('0:0,1,2,3 1:3,4,5 2:5,6,7,8',
        'd03204f3e5c3719fdfc75416fff9f69857791f62c2c7f4656d05912419ccc7ff'),
}


@pytest.mark.parametrize('op,lanes,cut', CASES, ids=['%s-%d-%s' % c for c in CASES])
def test_call_plan(tmp_path, monkeypatch, op, lanes, cut):
    plan, digest, log = _run(tmp_path, monkeypatch, op, lanes, cut)
    want_plan, want_digest = EXPECTED['%s-%d-%s' % (op, lanes, cut)]
    assert plan == want_plan
    assert digest == want_digest
    calls = [c for batch in log for c in batch]
    assert calls and all(c[0] == ('rank_hist' if op in ('quantile', 'mad') else 'gram' if op == 'cov' else op) for c in calls)
    if cut == 'resident':
        lens = [n for c in calls for n in c[6]]
        assert 0 in lens and any(lens)                            # some chunks go without bytes, some with
    if op == 'detect':
        assert any(c[-1] > 7 for c in calls)                      # (the second call of a short buffer is in the plan)


if __name__ == '__main__':
    import pathlib
    import tempfile
    print('EXPECTED = {')
    for case in CASES:
        with tempfile.TemporaryDirectory() as d:
            mp = pytest.MonkeyPatch()
            try:
                plan, digest, _ = _run(pathlib.Path(d), mp, *case)
            finally:
                mp.undo()
        print('    %r: (%r,\n        %r),' % ('%s-%d-%s' % case, plan, digest))
    print('}')
