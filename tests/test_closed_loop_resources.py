"""The closed-loop kernels (fe_policy_io.h) in the shipped gfx950 code object use no scratch and spill no VGPR.  Reads the AMDGPU metadata
notes of the code object inside the built libfluidengine_hip.so (scripts/kres.py --lib), as tests/test_render_resources.py does: no GPU, no
recompilation."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICY_KERNELS = ['k_obs_scatter_grad<0>', 'k_eff_add_state_grad<0>', 'k_eff_set_action_dev<0>']


@pytest.fixture(scope='module')
def kres():
    import __graft_entry__ as g
    g.build()                                                 # (up to date unless the sources changed)
    spec = importlib.util.spec_from_file_location('kres', os.path.join(ROOT, 'scripts', 'kres.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_closed_loop_kernels_use_no_scratch(kres):
    res = kres.kernel_resources()
    missing = [k for k in POLICY_KERNELS if k not in res]
    assert not missing, f'kernels not found in the code object: {missing}'
    bad = {k: res[k] for k in POLICY_KERNELS if res[k]['scratch'] != 0 or res[k]['vgpr_spills'] != 0}
    assert not bad, f'scratch / VGPR spills in the closed-loop kernels: {bad}'
    # one thread per distinct particle, one word per lane: nothing here may hold a wave back
    over = {k: res[k]['vgpr'] for k in POLICY_KERNELS if res[k]['vgpr'] > 64}
    assert not over, over


def test_closed_loop_kernels_sit_behind_the_plain_kernels(kres):
    """template instantiations are emitted behind every plain kernel: the new ones do not come between two plain kernels of the parent,
    nor between two kernels of the 16 KB-aligned substep group"""
    addr = kres.kernel_addresses()
    first, last = min(addr[k][0] for k in POLICY_KERNELS), max(addr[k][0] + addr[k][1] for k in POLICY_KERNELS)
    assert addr['k_render_shade'][0] < first and addr['k_mesh_sdf'][0] < first and addr['k_obs_gather'][0] < first
    aligned = [addr[k][0] for k in ('k_p2g<true, false>', 'k_g2p_p2g<false>', 'k_pgg_g2pg<4, false>', 'k_grid<false, false, false>', 'k_g2p<false>',
                                    'k_g2p_grad2<4>', 'k_grid_grad<false, false>', 'k_p2g_grad<false, 4>')]
    assert last <= min(aligned) or first >= max(aligned), (hex(first), hex(last), [hex(v) for v in aligned])
