"""The observation-field kernels (fe_field_obs.h) in the shipped gfx950 code object use no scratch, spill no VGPR and stay within register
budgets.  Reads the AMDGPU metadata notes of the code object inside the built libfluidengine_hip.so (scripts/kres.py --lib), as
tests/test_closed_loop_resources.py does: no GPU, no recompilation.

This build reports (VGPR / SGPR): k_field_obs_scatter<true> 44 / 86, k_field_obs_scatter<false> 44 / 88, k_field_obs_decode<0> 10 / 18,
k_field_obs_grad<0> 74 / 44; no AGPR, no scratch, no static LDS (the scatter's LDS is dynamic).  The budgets are the occupancy steps those
figures sit in: 64 VGPR keeps eight waves per SIMD for the scatter, whose LDS copies allow one workgroup per CU anyway, and for the
one-word-per-lane decode; 80 VGPR keeps six for the gather, which holds a 27-cell stencil in fp64."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = {'k_field_obs_scatter<true>': 64, 'k_field_obs_scatter<false>': 64, 'k_field_obs_decode<0>': 64, 'k_field_obs_grad<0>': 80}
KERNELS = list(BUDGET)


@pytest.fixture(scope='module')
def kres():
    import __graft_entry__ as g
    g.build()                                                 # (up to date unless the sources changed)
    spec = importlib.util.spec_from_file_location('kres', os.path.join(ROOT, 'scripts', 'kres.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_field_obs_kernels_use_no_scratch_and_keep_their_budgets(kres):
    res = kres.kernel_resources()
    missing = [k for k in KERNELS if k not in res]
    assert not missing, f'kernels not found in the code object: {missing}'
    print({k: (res[k]['vgpr'], res[k]['sgpr']) for k in KERNELS})
    bad = {k: res[k] for k in KERNELS if res[k]['scratch'] != 0 or res[k]['vgpr_spills'] != 0}
    assert not bad, f'scratch / VGPR spills in the observation-field kernels: {bad}'
    over = {k: res[k]['vgpr'] for k in KERNELS if res[k]['vgpr'] > BUDGET[k]}
    assert not over, over
    assert all(res[k]['sgpr'] <= 96 for k in KERNELS), {k: res[k]['sgpr'] for k in KERNELS}


def test_field_obs_kernels_are_the_last_code_of_the_object(kres):
    """template instantiations first used at the end of fe_engine.hip: behind every plain kernel, behind every other instantiation, and not
    between two kernels of the 16 KB-aligned substep group"""
    addr = kres.kernel_addresses()
    first, last = min(addr[k][0] for k in KERNELS), max(addr[k][0] + addr[k][1] for k in KERNELS)
    others = [k for k in addr if k not in KERNELS]
    behind = [k for k in others if addr[k][0] > first]
    aligned = [addr[k][0] for k in ('k_p2g<true, false>', 'k_g2p_p2g<false>', 'k_pgg_g2pg<4, false>', 'k_grid<false, false, false>', 'k_g2p<false>',
                                    'k_g2p_grad2<4>', 'k_grid_grad<false, false>', 'k_p2g_grad<false, 4>')]
    assert last <= min(aligned) or first >= max(aligned), (hex(first), hex(last), [hex(v) for v in aligned])
    for k in ('k_render_shade', 'k_obs_gather', 'k_obs_scatter_grad<0>', 'k_density_scatter<true>', 'k_task_pair<true>'):
        assert addr[k][0] < first, k
    print(f'{len(behind)} kernels behind the first observation-field kernel: {behind}')
