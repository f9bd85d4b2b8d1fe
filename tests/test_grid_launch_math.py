"""Host build of the grid kernels' launch chooser -- fe_grid_launch_wgs / fe_grid_launch_fixed of fluidlab_amd/csrc/fe_grid_launch.h, the function the engine sizes
every separate k_grid / k_grid_grad launch with -- checked over a sweep of list lengths x explicit caps x grid sizes x margins (tests/csrc/grid_launch_test.cpp):
a multiple of 128 wherever the cap and the grid allow, monotone in the length while one entry per wave is in reach, never above an explicit cap, the fixed 1,024
without a length, and 4 x result >= length below the one-entry-per-wave cap.  No GPU, no oracle."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'grid_launch_test.cpp')
OUT = os.path.join(ROOT, 'tests', 'csrc', '_build')


def test_grid_launch_math_host():
    cxx = shutil.which('g++') or shutil.which('clang++') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc'))
    if cxx is None:
        pytest.skip('no C++ compiler available')
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, 'grid_launch_test')
    subprocess.check_call([cxx, '-O2', '-std=c++17', '-x', 'c++', SRC, '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert ' 0 failures' in r.stdout
