"""Host build of the smoke reads' shared math -- fe_sl_value, fe_sl_grad, fe_ss_cell, the fixed-order merge and fe_ss_finish of
fluidlab_amd/csrc/fe_smoke_reads.h, the functions the kernels run on the device -- against plain fp64 loops
(tests/csrc/smoke_reads_test.cpp).  No GPU, no oracle."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'smoke_reads_test.cpp')
OUT = os.path.join(ROOT, 'tests', 'csrc', '_build')


def test_smoke_reads_math_host():
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    if hipcc is None:
        pytest.skip('hipcc not available')
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, 'smoke_reads_test')
    subprocess.check_call([hipcc, '--offload-host-only', '-O2', '-std=c++17', '-x', 'hip', SRC, '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '0 failures' in r.stdout
