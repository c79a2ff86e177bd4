"""Randomised safety of the leading-channel prefix decode under -m gpu: tools/fuzz_prefix_reads_gpu.py for MTS_FUZZ_CASES cases
(default 24) with a fixed seed (MTS_FUZZ_SEED overrides it; the seed is printed): dtype, flags, rows, leading count, stream writer
and prefix length drawn at random, every answer E_MISS or numpy's bytes.  Replay a failure with
    MTS_FUZZ_SEED=<seed> MTS_FUZZ_CASES=500 python -m pytest tests/test_gpu_prefix_reads_fuzz.py -m gpu -s
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

SEED = int(os.environ.get('MTS_FUZZ_SEED', 20261021))
CASES = int(os.environ.get('MTS_FUZZ_CASES', 24))


def test_fuzz_prefix_reads(tmp_path):
    env = dict(os.environ, PYTHONWARNINGS='ignore', HOME=str(tmp_path), TMPDIR=str(tmp_path))
    env.pop('MTSCOMP_DEVICE_CACHE_GB', None)
    print('fuzz_prefix_reads_gpu seed %d' % SEED)
    p = subprocess.run([sys.executable, str(ROOT / 'tools' / 'fuzz_prefix_reads_gpu.py'), str(SEED), str(CASES)], env=env, cwd=str(ROOT),
                       capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-3000:])
    assert p.returncode == 0, 'seed %d: %s' % (SEED, (p.stdout + p.stderr)[-3000:])
    assert p.stdout.rstrip().endswith(' 0 mismatches') and ' 0 cases' not in p.stdout, p.stdout[-500:]
