"""Host build of the density math -- the quadratic B-spline stencil, its derivative, the dropped cells, the guard and the fixed-point
deposit of fluidlab_amd/csrc/fe_density.h, the functions the k_density_* kernels and k_task_bwd run on the device -- against the
definition in plain loops (tests/csrc/density_test.cpp).  No GPU, no oracle."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'density_test.cpp')
OUT = os.path.join(ROOT, 'tests', 'csrc', '_build')


def test_density_math_host():
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    if hipcc is None:
        pytest.skip('hipcc not available')
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, 'density_test')
    subprocess.check_call([hipcc, '--offload-host-only', '-O2', '-std=c++17', '-x', 'hip', SRC, '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '0 failures' in r.stdout
