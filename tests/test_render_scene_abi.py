"""The scene calls of the renderer (include/fluidengine_ext.h: fe_render_set_volume, fe_render_set_scene, fe_render_scene_frame): declared in
the header, exported by the built HIP library, bound in _capi with a ctypes mirror of FeRenderScene that has the layout of the C struct;
the id ranges of particles, point sets, volumes and cells do not overlap; an oracle engine refuses the calls.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from fluidlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(__file__))
import render_scene_ref as RS  # noqa: E402

NAMES = ['fe_render_set_volume', 'fe_render_set_scene', 'fe_render_scene_frame']


def test_names_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'fluidengine_ext.h')).read()
    for n in NAMES:
        assert re.search(r'^(?:extern )?int %s\(FeEngine\* h, ' % n, text, re.M), n
        assert n in _capi.EXT_SYMBOLS and n not in _capi.ABI_SYMBOLS
        assert hasattr(_capi.Engine, n[3:]), n
    import __graft_entry__ as g
    g.build()                                                    # (up to date unless the sources changed)
    lib = _capi.load_hip()
    assert [s for s in NAMES if not hasattr(lib.lib, s)] == []
    assert lib.has_ext and lib.missing_symbols() == []
    block = text[text.index('The scene in that picture'):text.index('#ifndef FLUIDENGINE_EXT_H')]
    for word in ('Contract', 'Errors', 'Out of scope', 'SIGN', 'march_step', 'bisect_iters', 'thinner than', 'Rinv', 'transparency'):
        assert word in block, word
    srcs = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert "'fe_render_scene.h'" in srcs
    eng = open(os.path.join(ROOT, 'fluidlab_amd', 'csrc', 'fe_engine.hip')).read()
    assert eng.index('#include "fe_render.h"') < eng.index('#include "fe_render_scene.h"') < eng.index('int fe_real_size(void)')
    assert len(re.findall(r'^#include "fe_\w+\.h"', eng[eng.index('#include "fe_render_scene.h"') + 10:], re.M)) == 0       # nothing behind it


def test_ctypes_struct_has_the_layout_of_the_c_struct(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or ('/opt/rocm/llvm/bin/clang' if os.path.exists('/opt/rocm/llvm/bin/clang') else None)
    if cc is None:
        pytest.skip('no C compiler')
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fluidengine_ext.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(FeRenderScene), offsetof(FeRenderScene, smoke_radius),\n'
                   '    offsetof(FeRenderScene, cold), offsetof(FeRenderScene, hot), offsetof(FeRenderScene, bisect_iters), offsetof(FeRenderScene, draw_smoke),\n'
                   '    offsetof(FeRenderScene, lo), offsetof(FeRenderScene, hi), FE_RENDER_MAX_VOLUMES, FE_RENDER_VOL_NONE, FE_RENDER_VOL_STATIC,\n'
                   '    FE_RENDER_VOL_EFFECTOR, FE_RENDER_VOL_OWN, FE_RENDER_MAX_SETS * FE_RENDER_MAX_POINTS);\n'
                   '    return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Sc = _capi.FeRenderScene
    assert [ctypes.sizeof(Sc), Sc.smoke_radius.offset, Sc.cold.offset, Sc.hot.offset, Sc.bisect_iters.offset, Sc.draw_smoke.offset, Sc.lo.offset, Sc.hi.offset] \
        == out[:8] == [80, 8, 16, 40, 64, 68, 72, 76]
    assert out[8:13] == [_capi.FE_RENDER_MAX_VOLUMES, _capi.FE_RENDER_VOL_NONE, _capi.FE_RENDER_VOL_STATIC, _capi.FE_RENDER_VOL_EFFECTOR, _capi.FE_RENDER_VOL_OWN] == [16, 0, 1, 2, 3]
    assert out[13] == _capi.FE_RENDER_MAX_SETS * _capi.FE_RENDER_MAX_POINTS == RS.MAX_SETS * RS.MAX_POINTS
    hdr = open(os.path.join(ROOT, 'fluidlab_amd', 'csrc', 'fe_render_scene.h')).read()
    assert int(re.search(r'#define FE_RENDER_MAX_MARCH (\d+)', hdr).group(1)) == _capi.FE_RENDER_MAX_MARCH == RS.MAX_MARCH


def _ranges(N, n_grid):
    v0, c0 = RS.vol_id0(N), RS.cell_id0(N)
    return [(0, N), (N, N + _capi.FE_RENDER_MAX_SETS * _capi.FE_RENDER_MAX_POINTS), (v0, v0 + _capi.FE_RENDER_MAX_VOLUMES), (c0, c0 + n_grid ** 3)]


def test_id_ranges_do_not_overlap():
    """particles, point sets, volumes, cells: back to back, for no particles and for the largest grid fe_render_set_scene accepts (the
    largest id still fits a positive int; one more cell per axis does not)"""
    assert RS.vol_id0(0) == 2 * (1 << 20) and RS.cell_id0(0) == 2 * (1 << 20) + 16
    n_max = int(np.floor((2 ** 31 - RS.cell_id0(0)) ** (1.0 / 3.0)))
    while RS.cell_id0(0) + (n_max + 1) ** 3 - 1 <= 2 ** 31 - 1:
        n_max += 1
    while RS.cell_id0(0) + n_max ** 3 - 1 > 2 ** 31 - 1:
        n_max -= 1
    assert n_max == 1289
    for N, n in ((0, 16), (0, n_max), (1000000, 128), (300, 16)):
        r = _ranges(N, n)
        for (a0, a1), (b0, b1) in zip(r[:-1], r[1:]):
            assert a0 <= a1 == b0 <= b1
        assert r[-1][1] - 1 <= 2 ** 31 - 1
    assert RS.cell_id0(0) + (n_max + 1) ** 3 - 1 > 2 ** 31 - 1


def test_scene_calls_raise_on_an_oracle_engine(oracle64):
    import scenarios as S
    eng = S.make_engine(oracle64, S.water_block(n_grid=8, n_particles=8))
    for call in (lambda: eng.render_set_volume(0), lambda: eng.render_set_scene(None), lambda: eng.render_scene_frame(0, 0)):
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    eng.close()


def test_enable_scene_needs_a_renderer(oracle64):
    import test_host_env as H
    env = H._small('LatteArt-v0', oracle64, horizon=4, horizon_action=4, n_pool=300)
    with pytest.raises(AssertionError, match='No renderer available.'):
        env.enable_scene_render()
