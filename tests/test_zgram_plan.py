"""The slab arithmetic of the filtered Gram (csrc/reduce_plan.h: the groups of the grid, their Gram slabs and the z slabs those go
through) has no HIP in it.  tests/zgram_plan_check.cpp sweeps it on the CPU, built with the address and undefined-behaviour
sanitizers as a program of its own; this test builds it and runs it as a child process.  No GPU."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'mtscomp_amd' / 'csrc'


def test_zgram_plan_check_passes():
    build = subprocess.run(['make', '-C', str(CSRC), 'zgram_plan_check', 'BUILD=build'], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-4000:]
    run = subprocess.run([str(CSRC / 'build' / 'zgram_plan_check')], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert 'passed' in run.stdout
