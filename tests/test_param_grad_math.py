"""Host build (fp64) of the material-parameter adjoint's math -- constitutive_param_grad of fe_math.h and the node sums k_param_grad forms --
against finite differences of one particle's p2g deposit (tests/csrc/param_grad_test.cpp).  No GPU, no oracle."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'param_grad_test.cpp')
OUT = os.path.join(ROOT, 'tests', 'csrc', '_build')


def test_param_grad_math_host():
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    if hipcc is None:
        pytest.skip('hipcc not available')
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, 'param_grad_test_double')
    subprocess.check_call([hipcc, '--offload-host-only', '-O2', '-std=c++17', '-DFE_T=double', '-x', 'hip', SRC, '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '0 failures' in r.stdout
