"""The renderer's kernels in the shipped gfx950 code object use no scratch and spill no VGPR.  Reads the AMDGPU metadata notes of the code
object inside the built libfluidengine_hip.so (scripts/kres.py --lib), as tests/test_build_resources.py does for the substep kernels: no
GPU, no recompilation."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDER_KERNELS = ['k_render_clear', 'k_render_splat', 'k_render_points', 'k_render_shade']


@pytest.fixture(scope='module')
def kres():
    import __graft_entry__ as g
    g.build()                                                 # (up to date unless the sources changed)
    spec = importlib.util.spec_from_file_location('kres', os.path.join(ROOT, 'scripts', 'kres.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_render_kernels_do_not_spill(kres):
    res = kres.kernel_resources()
    missing = [k for k in RENDER_KERNELS if k not in res]
    assert not missing, f'kernels not found in the code object: {missing}'
    bad = {k: res[k] for k in RENDER_KERNELS if res[k]['scratch'] != 0 or res[k]['vgpr_spills'] != 0}
    assert not bad, f'scratch / VGPR spills in the render kernels: {bad}'
    # one wave per sphere at the worst: the splats must leave room for at least four waves per SIMD
    over = {k: res[k]['vgpr'] for k in RENDER_KERNELS if res[k]['vgpr'] > 128}
    assert not over, over


def test_render_kernels_follow_the_other_extension_kernels(kres):
    """fe_render.h is included after every other piece of device code: its kernels sit behind the other unaligned kernels of the source and
    do not come between two kernels of the 16 KB-aligned substep group"""
    addr = kres.kernel_addresses()
    first, last = min(addr[k][0] for k in RENDER_KERNELS), max(addr[k][0] + addr[k][1] for k in RENDER_KERNELS)
    assert addr['k_smoke_summary_merge'][0] < first and addr['k_mesh_sdf'][0] < first
    aligned = [addr[k][0] for k in ('k_p2g<true, false>', 'k_g2p_p2g<false>', 'k_pgg_g2pg<4, false>', 'k_grid<false, false, false>', 'k_g2p<false>',
                                    'k_g2p_grad2<4>', 'k_grid_grad<false, false>', 'k_p2g_grad<false, 4>')]
    assert last <= min(aligned) or first >= max(aligned), (hex(first), hex(last), [hex(v) for v in aligned])
