"""The rank arithmetic of the one-pass hash sort's scatter (csrc/op_rank.h, shared with k_op_scatter) has no HIP in it.
tests/scatter_rank_check.cpp replays a slice of 16 waves x 8 instructions x 64 lanes on the CPU, the lane-ordered LDS atomics as a
loop over the lanes, built with the address and undefined-behaviour sanitizers as a program of its own; this test builds it and runs
it as a child process.  No GPU."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'mtscomp_amd' / 'csrc'


def test_scatter_rank_check_passes():
    build = subprocess.run(['make', '-C', str(CSRC), 'scatter_rank_check', 'BUILD=build'], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-4000:]
    run = subprocess.run([str(CSRC / 'build' / 'scatter_rank_check')], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert 'all cases passed' in run.stdout
