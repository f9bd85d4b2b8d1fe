"""The kernels of the liquid surface (fluidlab_amd/csrc/fe_surface.h) in the shipped gfx950 code object use no scratch, spill no VGPR and hold
at most 128 VGPRs; k_surface_smooth holds its 32 x 32 tile in LDS; they are the last code of the object, behind the scene kernels of the
renderer, the field observations and the whole 16 KB-aligned substep group, as tests/test_render_scene_resources.py checks for the scene
kernels.  Reads the AMDGPU metadata of the built library (scripts/kres.py --lib): no GPU, no recompilation."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE_KERNELS = ['k_surface_opaque<0>', 'k_surface_splat<0>', 'k_surface_depth<0>', 'k_surface_smooth<0>', 'k_surface_shade<0>', 'k_surface_thickness<0>']
ALIGNED = ('k_p2g<true, false>', 'k_g2p_p2g<false>', 'k_pgg_g2pg<4, false>', 'k_grid<false, false, false>', 'k_g2p<false>',
           'k_g2p_grad2<4>', 'k_grid_grad<false, false>', 'k_p2g_grad<false, 4>')


@pytest.fixture(scope='module')
def kres():
    import __graft_entry__ as g
    g.build()                                                 # (up to date unless the sources changed)
    spec = importlib.util.spec_from_file_location('kres', os.path.join(ROOT, 'scripts', 'kres.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_surface_kernels_do_not_spill(kres):
    res = kres.kernel_resources()
    missing = [k for k in SURFACE_KERNELS if k not in res]
    assert not missing, f'kernels not found in the code object: {missing}'
    bad = {k: res[k] for k in SURFACE_KERNELS if res[k]['scratch'] != 0 or res[k]['vgpr_spills'] != 0}
    assert not bad, f'scratch / VGPR spills in the surface kernels: {bad}'
    over = {k: res[k]['vgpr'] for k in SURFACE_KERNELS if res[k]['vgpr'] > 128}
    assert not over, over
    assert res['k_surface_smooth<0>']['lds'] == 32 * 32 * 4
    assert all(res[k]['lds'] == 0 for k in SURFACE_KERNELS if k != 'k_surface_smooth<0>')


def test_surface_kernels_come_last(kres):
    addr = kres.kernel_addresses()
    first = min(addr[k][0] for k in SURFACE_KERNELS)
    others = {k: v for k, v in addr.items() if k not in SURFACE_KERNELS}
    assert all(a + n <= first for a, n in others.values()), [k for k, (a, n) in others.items() if a + n > first]
    assert first > max(addr[k][0] for k in ALIGNED)
    assert first > max(addr[k][0] for k in ('k_render_shade', 'k_render_shade_scene<0>', 'k_field_obs_grad<0>'))
