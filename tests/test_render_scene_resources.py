"""The three scene kernels of the renderer in the shipped gfx950 code object use no scratch, spill no VGPR and hold at most 128 VGPRs; they
lie behind k_render_shade and not between two kernels of the 16 KB-aligned substep group; and the four kernels of the particle renderer
are where tests/test_render_resources.py wants them (its placement assertion, repeated here so that a move shows up in this file too).
Reads the AMDGPU metadata of the built library (scripts/kres.py --lib): no GPU, no recompilation."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_KERNELS = ['k_render_smoke<0>', 'k_render_sdf<0>', 'k_render_shade_scene<0>']     # (templates with one instantiation: emitted at the tail, fe_render_scene.h)
RENDER_KERNELS = ['k_render_clear', 'k_render_splat', 'k_render_points', 'k_render_shade']
ALIGNED = ('k_p2g<true, false>', 'k_g2p_p2g<false>', 'k_pgg_g2pg<4, false>', 'k_grid<false, false, false>', 'k_g2p<false>',
           'k_g2p_grad2<4>', 'k_grid_grad<false, false>', 'k_p2g_grad<false, 4>')


@pytest.fixture(scope='module')
def kres():
    import __graft_entry__ as g
    g.build()                                                 # (up to date unless the sources changed)
    spec = importlib.util.spec_from_file_location('kres', os.path.join(ROOT, 'scripts', 'kres.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_scene_kernels_do_not_spill(kres):
    res = kres.kernel_resources()
    missing = [k for k in SCENE_KERNELS if k not in res]
    assert not missing, f'kernels not found in the code object: {missing}'
    bad = {k: res[k] for k in SCENE_KERNELS if res[k]['scratch'] != 0 or res[k]['vgpr_spills'] != 0}
    assert not bad, f'scratch / VGPR spills in the scene kernels: {bad}'
    over = {k: res[k]['vgpr'] for k in SCENE_KERNELS if res[k]['vgpr'] > 128}
    assert not over, over


def test_scene_kernels_come_last(kres):
    addr = kres.kernel_addresses()
    first = min(addr[k][0] for k in SCENE_KERNELS)
    last = max(addr[k][0] + addr[k][1] for k in SCENE_KERNELS)
    assert addr['k_render_shade'][0] + addr['k_render_shade'][1] <= first
    assert all(addr[k][0] < first for k in RENDER_KERNELS)
    aligned = [addr[k][0] for k in ALIGNED]
    assert last <= min(aligned) or first >= max(aligned), (hex(first), hex(last), [hex(v) for v in aligned])
    # behind the whole substep group and the smoke solver: nothing of either moved to make room
    assert first > max(aligned) and first > max(a for k, (a, _) in addr.items() if k.startswith('k_smoke_'))


def test_particle_render_kernels_keep_their_place(kres):
    """tests/test_render_resources.py's placement assertion for the four kernels of fe_render.h"""
    addr = kres.kernel_addresses()
    first, last = min(addr[k][0] for k in RENDER_KERNELS), max(addr[k][0] + addr[k][1] for k in RENDER_KERNELS)
    assert addr['k_smoke_summary_merge'][0] < first and addr['k_mesh_sdf'][0] < first
    aligned = [addr[k][0] for k in ALIGNED]
    assert last <= min(aligned) or first >= max(aligned), (hex(first), hex(last), [hex(v) for v in aligned])
