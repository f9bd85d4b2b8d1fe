"""The liquid-surface calls of the renderer (include/fluidengine_ext.h: fe_surface_set, fe_surface_frame, fe_surface_get, fe_surface_get_dev):
declared in the header, exported by the built HIP library, bound in _capi with a ctypes mirror of FeSurfaceParams that has the layout of the
C struct; the header documents contract, errors and scope; the new header is part of the library's sources; an oracle engine and an
oracle-backed environment refuse the calls.  No GPU needed."""
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

NAMES = ['fe_surface_set', 'fe_surface_frame', 'fe_surface_get', 'fe_surface_get_dev']


def test_names_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'fluidengine_ext.h')).read()
    assert sorted(set(re.findall(r'^extern int (fe_surface_\w+)\(FeEngine\* h, ', text, re.M))) == sorted(NAMES)
    for n in NAMES:
        assert n in _capi.EXT_SYMBOLS and n not in _capi.ABI_SYMBOLS
        assert hasattr(_capi.Engine, n[3:]), n
    import __graft_entry__ as g
    g.build()                                                    # (up to date unless the sources changed)
    lib = _capi.load_hip()
    assert [s for s in NAMES if not hasattr(lib.lib, s)] == []
    assert lib.has_ext and lib.missing_symbols() == []
    block = text[text.index('Liquids in that picture'):text.index('#ifndef FLUIDENGINE_EXT_H')]
    for word in ('Contract', 'Errors', 'Out of scope', 'Read-only', 'Deterministic', 'radius_scale', 'smooth_iters', 'smooth_radius_px', 'range', 'absorb', 'alpha_min',
                 'specular', 'shininess_log2', 'atomicMin', '2^32', 'refraction', 'fe_render_scene_frame'):
        assert word in block, word
    assert "'fe_surface.h'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert os.path.join(g.CSRC, 'fe_surface.h') in g.engine_sources()      # an edit to it rebuilds the library
    scene_h = open(os.path.join(ROOT, 'fluidlab_amd', 'csrc', 'fe_render_scene.h')).read()
    assert scene_h.index('#include "fe_surface.h"') < scene_h.index('#endif /* FE_RENDER_MATH_ONLY */')
    assert '#include "fe_surface.h"' not in open(os.path.join(ROOT, 'fluidlab_amd', 'csrc', 'fe_engine.hip')).read()


def test_ctypes_struct_has_the_layout_of_the_c_struct(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or ('/opt/rocm/llvm/bin/clang' if os.path.exists('/opt/rocm/llvm/bin/clang') else None)
    if cc is None:
        pytest.skip('no C compiler')
    fields = [n for n, _ in _capi.FeSurfaceParams._fields_]
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fluidengine_ext.h"\n'
                   'int main(void) { printf("%zu' + ' %zu' * len(fields) + '\\n", sizeof(FeSurfaceParams), '
                   + ', '.join(f'offsetof(FeSurfaceParams, {n})' for n in fields) + ');\n    return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _capi.FeSurfaceParams
    assert [ctypes.sizeof(P)] + [getattr(P, n).offset for n in fields] == out == [56, 0, 8, 16, 24, 32, 40, 44, 48, 52]
    assert fields == ['radius_scale', 'range', 'absorb', 'alpha_min', 'specular', 'smooth_iters', 'smooth_radius_px', 'shininess_log2', 'pad']
    hdr = open(os.path.join(ROOT, 'fluidlab_amd', 'csrc', 'fe_surface.h')).read()
    assert int(re.search(r'#define FE_SURFACE_TILE (\d+)', hdr).group(1)) == 16 and int(re.search(r'#define FE_SURFACE_MAX_R (\d+)', hdr).group(1)) == 8


def test_renderer_defaults_are_inside_the_ranges():
    from fluidlab_amd.fluidengine.renderers import hip_renderer as HR
    d = HR.LIQUID_SURFACE_DEFAULTS
    assert set(d) == {n for n, _ in _capi.FeSurfaceParams._fields_} - {'pad'}
    assert d['radius_scale'] == 1.5 and d['smooth_iters'] == 2 and d['smooth_radius_px'] == 5
    assert 0 <= d['alpha_min'] <= 1 and 0 <= d['specular'] <= 1 and 0 <= d['shininess_log2'] <= 10 and d['absorb'] >= 0


def test_surface_calls_raise_on_an_oracle_engine(oracle64):
    import scenarios as S
    eng = S.make_engine(oracle64, S.water_block(n_grid=8, n_particles=8))
    calls = [lambda: eng.surface_set(np.ones(8, np.uint8), _capi.FeSurfaceParams()), lambda: eng.surface_set(None), lambda: eng.surface_frame(0, 0),
             lambda: eng.surface_get(), lambda: eng.surface_get_dev()]
    for call in calls:
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    eng.close()


def test_enable_liquid_surface_needs_a_renderer(oracle64):
    import test_host_env as H
    env = H._small('LatteArt-v0', oracle64, horizon=4, horizon_action=4, n_pool=300)
    with pytest.raises(AssertionError, match='No renderer available.'):
        env.enable_liquid_surface()
    with pytest.raises(AssertionError, match='No renderer available.'):
        env.taichi_env.render_surface_buffers()
