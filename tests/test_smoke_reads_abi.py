"""The smoke-field reads are HIP-engine extensions (include/fluidengine_ext.h): the header compiles as C, the ctypes mirror of FeSmokeSummary has
the layout of the C struct, the constants agree, the HIP library exports the ten names, FeLossTerm keeps its 72 bytes and no term kind 7
appeared, and an oracle engine refuses the new calls.  No GPU needed."""
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

NAMES = ['fe_smoke_cells_set', 'fe_smoke_cells_get', 'fe_smoke_cells_get_dev', 'fe_smoke_loss_alloc', 'fe_smoke_loss_set', 'fe_smoke_loss_clear',
         'fe_smoke_loss_step', 'fe_smoke_loss_step_grad', 'fe_smoke_loss_get', 'fe_smoke_summary']


def test_hip_library_exports_the_ten_names():
    if not os.path.exists(_capi.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _capi.load_hip()
    assert set(NAMES) <= set(_capi.EXT_SYMBOLS)
    assert [s for s in NAMES if not hasattr(lib.lib, s)] == []
    assert lib.has_ext and lib.missing_symbols() == []
    assert not set(NAMES) & set(_capi.ABI_SYMBOLS)


def test_header_compiles_as_c_and_the_mirror_has_its_layout(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or ('/opt/rocm/llvm/bin/clang' if os.path.exists('/opt/rocm/llvm/bin/clang') else None)
    if cc is None:
        pytest.skip('no C compiler')
    fields = ['n_cells', 'n_nonfinite', 'v_max', 'courant', 'kinetic', 'q_sum', 'q_min', 'q_max']
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fluidengine_ext.h"\n'
                   'int main(void) { printf("%zu %zu", sizeof(FeSmokeSummary), sizeof(FeLossTerm));\n'
                   + ''.join(f'    printf(" %zu", offsetof(FeSmokeSummary, {f}));\n' for f in fields) +
                   '    printf(" %d %d %d %d", FE_SMOKE_MAX_LISTS, FE_SMOKE_MAX_LIST_CELLS, FE_SMOKE_L1, FE_SMOKE_SQ);\n'
                   '    printf(" %d %d %d %d %d\\n", FE_TERM_L1_CONST, FE_TERM_SQ_CONST, FE_TERM_L1_REF, FE_TERM_PAIR_L1, FE_TERM_DENSITY_SQ); return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.check_call([cc, '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _capi.FeSmokeSummary
    assert [n for n, _ in S._fields_] == fields
    assert ctypes.sizeof(S) == out[0] == 112
    assert ctypes.sizeof(_capi.FeLossTerm) == out[1] == 72
    assert [getattr(S, f).offset for f in fields] == out[2:10] == [0, 8, 16, 24, 32, 40, 64, 88]
    assert out[10:14] == [_capi.FE_SMOKE_MAX_LISTS, _capi.FE_SMOKE_MAX_LIST_CELLS, _capi.FE_SMOKE_L1, _capi.FE_SMOKE_SQ] == [4, 1 << 16, 0, 1]
    # the term kinds are still 0..4: 7 names nothing (existing tests hand kind 7 to fe_task_loss_set_terms as the unknown kind)
    kinds = [_capi.FE_TERM_L1_CONST, _capi.FE_TERM_SQ_CONST, _capi.FE_TERM_L1_REF, _capi.FE_TERM_PAIR_L1, _capi.FE_TERM_DENSITY_SQ]
    assert out[14:] == kinds == [0, 1, 2, 3, 4]
    assert [k for k in dir(_capi) if k.startswith('FE_TERM_') and getattr(_capi, k) == 7] == []


def test_new_engine_methods_raise_on_an_oracle_engine(oracle64):
    import scenarios as S
    eng = S.make_engine(oracle64, S.water_block(n_grid=8, n_particles=8))
    calls = [lambda: eng.smoke_cells_set(0, np.zeros((1, 3), np.int32)), lambda: eng.smoke_cells_get(0, 0), lambda: eng.smoke_cells_get_dev(0, 0),
             lambda: eng.smoke_loss_alloc(4), lambda: eng.smoke_loss_set(0, np.zeros(1)), lambda: eng.smoke_loss_clear(), lambda: eng.smoke_loss_step(0, 0),
             lambda: eng.smoke_loss_step_grad(0, 0, 1.0), lambda: eng.smoke_loss_get(1), lambda: eng.smoke_summary(0)]
    for call in calls:
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    eng.close()


def test_oracle_backed_circulation_refuses_the_device_roads(oracle64):
    import test_host_env as H
    env = H._circulation(oracle64, max_substeps_local=None)
    te = env.taichi_env
    for call in (env.enable_device_obs, env.enable_device_loss, te.enable_device_loss, te.loss.enable_device_loss, te.smoke_summary, te.smoke_field.summary):
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    assert not env._device_obs and not te.loss._device_loss
    obs, reward, done, info = env.step(np.zeros(env.agent.action_dim))             # ... and behaves as before
    assert np.isfinite(obs).all() and info == {}
