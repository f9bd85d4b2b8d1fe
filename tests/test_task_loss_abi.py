"""The loss-term programs are HIP-engine extensions (include/fluidengine_ext.h): the HIP library exports their seven names, the ctypes
mirror of FeLossTerm has the layout of the C struct, an oracle engine refuses every new Engine method and an oracle-backed environment
refuses enable_device_loss().  No GPU needed."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

from fluidlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(__file__))

NAMES = ['fe_task_loss_alloc', 'fe_task_loss_set_terms', 'fe_task_loss_set_ref', 'fe_task_loss_clear', 'fe_task_loss_step',
         'fe_task_loss_step_grad', 'fe_task_loss_get']


def test_hip_library_exports_the_seven_names():
    if not os.path.exists(_capi.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _capi.load_hip()
    assert set(NAMES) <= set(_capi.EXT_SYMBOLS)
    assert [s for s in NAMES if not hasattr(lib.lib, s)] == []
    assert lib.has_ext and lib.missing_symbols() == []
    assert not set(NAMES) & set(_capi.ABI_SYMBOLS)


def test_ctypes_term_has_the_layout_of_the_c_struct(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or ('/opt/rocm/llvm/bin/clang' if os.path.exists('/opt/rocm/llvm/bin/clang') else None)
    if cc is None:
        pytest.skip('no C compiler')
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fluidengine_ext.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(FeLossTerm), sizeof(FeLossSel), offsetof(FeLossTerm, b), offsetof(FeLossTerm, weight),\n'
                   '    FE_TASK_LOSS_MAX_TERMS, FE_TASK_LOSS_MAX_PAIR_TERMS, FE_TERM_L1_CONST, FE_TERM_SQ_CONST, FE_TERM_L1_REF, FE_TERM_PAIR_L1); return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    size, sel_size, off_b, off_w = out[:4]
    assert ctypes.sizeof(_capi.FeLossTerm) == size == 72 and ctypes.sizeof(_capi.FeLossSel) == sel_size == 16
    assert _capi.FeLossTerm.b.offset == off_b and _capi.FeLossTerm.weight.offset == off_w
    assert out[4:] == [_capi.FE_TASK_LOSS_MAX_TERMS, _capi.FE_TASK_LOSS_MAX_PAIR_TERMS, _capi.FE_TERM_L1_CONST, _capi.FE_TERM_SQ_CONST,
                       _capi.FE_TERM_L1_REF, _capi.FE_TERM_PAIR_L1]


def test_new_engine_methods_raise_on_an_oracle_engine(oracle64):
    import scenarios as S
    from fluidlab_amd.fluidengine.losses.term_program import AXIS_X, L1_CONST, Sel, Term
    eng = S.make_engine(oracle64, S.water_block(n_grid=8, n_particles=8))
    term = Term(L1_CONST, AXIS_X, Sel(0, 8))
    calls = [lambda: eng.task_loss_alloc(4), lambda: eng.task_loss_set_terms([term]), lambda: eng.task_loss_set_ref(0), lambda: eng.task_loss_clear(),
             lambda: eng.task_loss_step(0, 0), lambda: eng.task_loss_step_grad(0, 0, 1.0), lambda: eng.task_loss_get(4)]
    for call in calls:
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    eng.close()


def test_enable_device_loss_raises_on_an_oracle_backed_env(oracle64):
    import test_host_env as H
    env = H._small('Mixing-v0', oracle64, horizon=4)
    assert env.taichi_env.loss.device_terms() is not None
    for call in (env.enable_device_loss, env.taichi_env.enable_device_loss, env.taichi_env.loss.enable_device_loss):
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    assert not env.taichi_env.loss._device_loss
    from fluidlab_amd.fluidengine.losses.host_loss import HostLoss
    assert HostLoss.device_terms(env.taichi_env.loss) is None   # the base class has no program
