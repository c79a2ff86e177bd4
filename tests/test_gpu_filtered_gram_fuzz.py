"""Randomised parity of Reader.cov with taps= / reference= under -m gpu: tools/fuzz_filtered_gram_gpu.py for MTS_FUZZ_SECONDS (default 5)
with a fixed seed (MTS_FUZZ_SEED overrides it; the seed is printed): gram and sum bit for bit against cov of a float32 recording that
holds the filtered rows, and within the bound of tests/gram_oracle.py on the numpy restatement of them.  Replay a failure with
    MTS_FUZZ_SEED=<seed> MTS_FUZZ_SECONDS=30 python -m pytest tests/test_gpu_filtered_gram_fuzz.py -m gpu -s
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

SEED = int(os.environ.get('MTS_FUZZ_SEED', 20261021))
SECONDS = float(os.environ.get('MTS_FUZZ_SECONDS', 5))


def test_fuzz_filtered_gram(tmp_path):
    env = dict(os.environ, PYTHONWARNINGS='ignore', HOME=str(tmp_path))
    for name in ('MTSCOMP_DEVICE_CACHE_GB', 'MTS_PIPE_BYTES', 'MTS_ZGRAM_SLAB_BYTES'):
        env.pop(name, None)
    print('fuzz_filtered_gram_gpu seed %d' % SEED)
    p = subprocess.run([sys.executable, str(ROOT / 'tools' / 'fuzz_filtered_gram_gpu.py'), str(SEED), str(SECONDS)], env=env, cwd=str(ROOT),
                       capture_output=True, text=True, timeout=SECONDS + 600)
    print(p.stdout[-3000:], p.stderr[-3000:])
    assert p.returncode == 0, 'seed %d: %s' % (SEED, (p.stdout + p.stderr)[-3000:])
