"""The renderer is a HIP-engine extension (include/fluidengine_ext.h): the HIP library exports its six names, the ctypes mirrors of
FeRenderCamera and FeRenderLights have the layout of the C structs, an oracle engine and an oracle-backed environment refuse the calls, the
camera the Python side builds is orthonormal, and write_png writes a file that decodes back to the same bytes.  No GPU needed."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from fluidlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(__file__))

NAMES = ['fe_render_setup', 'fe_render_set_colors', 'fe_render_set_points', 'fe_render_frame', 'fe_render_get', 'fe_render_get_dev']


def test_hip_library_exports_the_six_names():
    if not os.path.exists(_capi.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _capi.load_hip()
    assert set(NAMES) <= set(_capi.EXT_SYMBOLS)
    assert [s for s in NAMES if not hasattr(lib.lib, s)] == []
    assert lib.has_ext and lib.missing_symbols() == []
    assert not set(NAMES) & set(_capi.ABI_SYMBOLS)


def test_binding_covers_the_header_block():
    """every fe_render_* the header declares is in EXT_SYMBOLS and has an Engine method, and the header documents contract, errors and scope"""
    import re
    text = open(os.path.join(ROOT, 'include', 'fluidengine_ext.h')).read()
    declared = sorted(set(re.findall(r'^int (fe_render_\w+)\(', text, re.M)))
    assert declared == sorted(NAMES)
    for n in declared:
        assert hasattr(_capi.Engine, n[3:]), n
    block = text[text.index('Headless particle renderer'):text.index('#ifndef FLUIDENGINE_EXT_H')]
    for word in ('Contract', 'Errors', 'Out of scope', 'meshes', 'shadows', 'transparency', 'anti-aliasing', 'smoke field', 'batched', "mode='human'", 'gradients'):
        assert word in block, word


def test_ctypes_structs_have_the_layout_of_the_c_structs(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or ('/opt/rocm/llvm/bin/clang' if os.path.exists('/opt/rocm/llvm/bin/clang') else None)
    if cc is None:
        pytest.skip('no C compiler')
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fluidengine_ext.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(FeRenderCamera), offsetof(FeRenderCamera, right),\n'
                   '    offsetof(FeRenderCamera, fwd), offsetof(FeRenderCamera, focal), offsetof(FeRenderCamera, max_radius_px), offsetof(FeRenderCamera, width),\n'
                   '    offsetof(FeRenderCamera, height), sizeof(FeRenderLights), offsetof(FeRenderLights, pos), offsetof(FeRenderLights, color),\n'
                   '    offsetof(FeRenderLights, n_lights), FE_RENDER_MAX_LIGHTS, FE_RENDER_MAX_SETS, FE_RENDER_MAX_POINTS, FE_RENDER_MAX_SIZE, FE_RENDER_LANE_PIXELS);\n'
                   '    return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Cm, L = _capi.FeRenderCamera, _capi.FeRenderLights
    assert [ctypes.sizeof(Cm), Cm.right.offset, Cm.fwd.offset, Cm.focal.offset, Cm.max_radius_px.offset, Cm.width.offset, Cm.height.offset] == out[:7] == [128, 24, 72, 96, 112, 120, 124]
    assert [ctypes.sizeof(L), L.pos.offset, L.color.offset, L.n_lights.offset] == out[7:11] == [248, 48, 144, 240]
    assert out[11:] == [_capi.FE_RENDER_MAX_LIGHTS, _capi.FE_RENDER_MAX_SETS, _capi.FE_RENDER_MAX_POINTS, _capi.FE_RENDER_MAX_SIZE, _capi.FE_RENDER_LANE_PIXELS] == [4, 2, 1 << 20, 4096, 25]


def test_render_calls_raise_on_an_oracle_engine(oracle64):
    import scenarios as S
    from fluidlab_amd.fluidengine.renderers import hip_renderer as HR
    eng = S.make_engine(oracle64, S.water_block(n_grid=8, n_particles=8))
    cam, lights = HR.make_camera((8, 8), (0.5, 0.5, 3), (0.5, 0.5, 0.5), 30), HR.make_lights([])
    calls = [lambda: eng.render_setup(cam, lights), lambda: eng.render_set_colors(np.zeros((8, 4), np.uint8), 0.01), lambda: eng.render_set_points(0, None),
             lambda: eng.render_frame(0), lambda: eng.render_get(), lambda: eng.render_get_dev()]
    for call in calls:
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    eng.close()


def test_oracle_backed_env_refuses_the_renderer_and_none_is_as_before(oracle64):
    import test_host_env as H
    with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
        H._small('LatteArt-v0', oracle64, horizon=4, horizon_action=4, n_pool=300, renderer_type='HIP')
    env = H._small('LatteArt-v0', oracle64, horizon=4, horizon_action=4, n_pool=300)
    assert env.renderer_type is None and env.taichi_env.renderer is None
    with pytest.raises(AssertionError, match='No renderer available.'):
        env.taichi_env.render()
    with pytest.raises(AssertionError, match='No renderer available.'):
        env.render('rgb_array')
    with pytest.raises(NotImplementedError):
        env.taichi_env.setup_renderer(type='GGUI')
    with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
        env.taichi_env.setup_renderer(type='HIP')
    assert env.taichi_env.renderer is None


def test_camera_basis_is_orthonormal_and_right_handed():
    from fluidlab_amd.fluidengine.renderers import hip_renderer as HR
    for pos, at in (((-0.15, 2.82, 2.5), (0.5, 0.5, 0.5)), ((0.5, 12.0, 0.501), (0.5, 0.5, 0.5)), ((4.48, 2.41, -0.84), (3.64, 1.95, -0.56))):
        r, u, f = HR.camera_basis(pos, at)
        M = np.stack([r, u, f])
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-14 and u[1] > 0
        assert np.abs(np.cross(r, f) - u).max() < 1e-14                          # as the engine's header has it: up = right x fwd
    cam = HR.make_camera((960, 640), (0.5, 0.5, 3.0), (0.5, 0.5, 0.5), 30)
    assert cam.width == 960 and cam.height == 640 and abs(cam.focal - 320 / np.tan(np.deg2rad(15))) < 1e-9 and cam.max_radius_px == 32.0
    assert list(cam.fwd) == [0.0, 0.0, -1.0] and list(cam.right) == [1.0, 0.0, 0.0] and list(cam.up) == [0.0, 1.0, 0.0]
    with pytest.raises(ValueError):
        HR.camera_basis((0.5, 3.0, 0.5), (0.5, 0.5, 0.5))                        # looking along `up`
    with pytest.raises(ValueError):
        HR.make_lights([{'pos': (0, 0, 0), 'color': (1, 1, 1)}] * 5)
    assert np.array_equal(HR.colors_to_bytes(np.array([[0.0, 0.5, 1.0, 2.0]])), [[0, 128, 255, 255]])


def _chunks(data):
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    p, out = 8, []
    while p < len(data):
        n, kind = struct.unpack('>I4s', data[p:p + 8])
        body = data[p + 8:p + 8 + n]
        crc, = struct.unpack('>I', data[p + 8 + n:p + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        out.append((kind, body))
        p += 12 + n
    assert p == len(data)
    return out


@pytest.mark.parametrize('shape', [(5, 7, 3), (1, 1, 3), (16, 3, 4)])
def test_write_png_round_trip(tmp_path, shape):
    from fluidlab_amd.utils.image import write_png
    img = np.random.RandomState(0).randint(0, 256, shape).astype(np.uint8)
    path = tmp_path / 'a.png'
    write_png(str(path), img)
    chunks = _chunks(path.read_bytes())
    assert [k for k, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    H, W, ch = shape
    assert struct.unpack('>IIBBBBB', chunks[0][1]) == (W, H, 8, 2 if ch == 3 else 6, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(H, 1 + W * ch)
    assert np.all(raw[:, 0] == 0) and np.array_equal(raw[:, 1:].reshape(shape), img)
    with pytest.raises(ValueError):
        write_png(str(path), img.astype(np.float32))
