"""Target clouds and the Chamfer terms are HIP-engine extensions (include/fluidengine_ext.h): the HIP library exports the two new names, the
constants of the ctypes mirror are the header's, FeLossTerm keeps its 72 bytes and kind 7 stays free, and an oracle engine refuses the new
calls.  No GPU needed."""
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

NAMES = ['fe_cloud_set', 'fe_cloud_query']


def test_hip_library_exports_the_two_names():
    if not os.path.exists(_capi.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _capi.load_hip()
    assert set(NAMES) <= set(_capi.EXT_SYMBOLS)
    assert [s for s in NAMES if not hasattr(lib.lib, s)] == []
    assert lib.has_ext and lib.missing_symbols() == []
    assert not set(NAMES) & set(_capi.ABI_SYMBOLS)


def test_constants_and_struct_size_are_the_headers(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or ('/opt/rocm/llvm/bin/clang' if os.path.exists('/opt/rocm/llvm/bin/clang') else None)
    if cc is None:
        pytest.skip('no C compiler')
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include "fluidengine_ext.h"\n'
                   'int main(void) { printf("%zu %d %d %d %d %d %d %.17g\\n", sizeof(FeLossTerm), FE_TERM_NEAREST_SQ, FE_TERM_COVER_SQ, FE_TASK_LOSS_MAX_NEAREST_TERMS,\n'
                   '    FE_CLOUD_MAX, FE_CLOUD_MAX_POINTS, FE_TASK_LOSS_MAX_TERMS, (double)FE_CLOUD_COORD_MAX); return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert ctypes.sizeof(_capi.FeLossTerm) == int(out[0]) == 72
    assert [int(t) for t in out[1:7]] == [_capi.FE_TERM_NEAREST_SQ, _capi.FE_TERM_COVER_SQ, _capi.FE_TASK_LOSS_MAX_NEAREST_TERMS, _capi.FE_CLOUD_MAX,
                                          _capi.FE_CLOUD_MAX_POINTS, _capi.FE_TASK_LOSS_MAX_TERMS] == [5, 6, 2, 4, 1 << 20, 8]
    assert float(out[7]) == _capi.FE_CLOUD_COORD_MAX == 2.0
    kinds = [_capi.FE_TERM_L1_CONST, _capi.FE_TERM_SQ_CONST, _capi.FE_TERM_L1_REF, _capi.FE_TERM_PAIR_L1, _capi.FE_TERM_DENSITY_SQ, _capi.FE_TERM_NEAREST_SQ,
             _capi.FE_TERM_COVER_SQ]
    assert kinds == list(range(7))                             # 7 is no kind


def test_term_packs_the_cloud_id():
    from fluidlab_amd.fluidengine.losses.term_program import AXIS_X, AXIS_Z, COVER_SQ, NEAREST_SQ, Sel, Term
    for kind in (NEAREST_SQ, COVER_SQ):
        t = Term(kind, AXIS_X | AXIS_Z, Sel(0, 5, 2, True), weight=-2.0, cloud=3).to_c()
        assert (t.kind, t.axis_mask, t.b.pid_lo, t.b.pid_hi, t.b.mat, t.b.require_used, t.weight) == (kind, 5, 3, 0, 0, 0, -2.0)
        assert (t.a.pid_lo, t.a.pid_hi, t.a.mat, t.a.require_used) == (0, 5, 2, 1)


def test_new_engine_methods_raise_on_an_oracle_engine(oracle64):
    import scenarios as S
    eng = S.make_engine(oracle64, S.water_block(n_grid=8, n_particles=8))
    pts = np.full((5, 3), 0.5, np.float32)
    for call in (lambda: eng.cloud_set(0, pts), lambda: eng.cloud_set(0, None), lambda: eng.cloud_query(0, 0)):
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    eng.close()
