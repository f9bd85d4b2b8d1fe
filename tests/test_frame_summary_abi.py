"""The observation gather and the frame summary are HIP-engine extensions (include/fluidengine_ext.h): the HIP library exports their five
names, the ctypes record has the size of the C one, and an oracle engine refuses every new Engine method.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from fluidlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(__file__))

NAMES = ['fe_obs_set_particles', 'fe_obs_get', 'fe_obs_get_dev', 'fe_summary_set_groups', 'fe_frame_summary']


def test_hip_library_exports_the_five_names():
    if not os.path.exists(_capi.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _capi.load_hip()
    assert set(NAMES) <= set(_capi.EXT_SYMBOLS)
    assert [s for s in NAMES if not hasattr(lib.lib, s)] == []
    assert lib.has_ext and lib.missing_symbols() == []
    assert not set(NAMES) & set(_capi.ABI_SYMBOLS)


def test_ctypes_record_has_the_size_of_the_c_struct(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or ('/opt/rocm/llvm/bin/clang' if os.path.exists('/opt/rocm/llvm/bin/clang') else None)
    if cc is None:
        pytest.skip('no C compiler')
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fluidengine_ext.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d\\n", sizeof(FeFrameSummary), offsetof(FeFrameSummary, courant), offsetof(FeFrameSummary, J_max), FE_SUMMARY_MAX_GROUPS); return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    size, off_courant, off_jmax, max_groups = (int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert ctypes.sizeof(_capi.FeFrameSummary) == size == 8 * 20
    assert _capi.FeFrameSummary.courant.offset == off_courant and _capi.FeFrameSummary.J_max.offset == off_jmax
    assert _capi.FE_SUMMARY_MAX_GROUPS == max_groups


def test_new_engine_methods_raise_on_an_oracle_engine(oracle64):
    import scenarios as S
    eng = S.make_engine(oracle64, S.water_block(n_grid=8, n_particles=8))
    calls = [lambda: eng.obs_set_particles([0, 1]), lambda: eng.get_obs(0), lambda: eng.get_obs_dev(0),
             lambda: eng.summary_set_groups(np.zeros(8, np.int32), 1), lambda: eng.frame_summary(0)]
    for call in calls:
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    eng.close()
