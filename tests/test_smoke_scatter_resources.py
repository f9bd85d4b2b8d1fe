"""The cell-list scatter kernel (fe_smoke_reads.h) in the shipped gfx950 code object uses no scratch, spills no VGPR and sits behind the plain
kernels, outside the aligned substep group.  Reads the AMDGPU metadata notes of the code object inside the built libfluidengine_hip.so
(scripts/kres.py --lib), as tests/test_closed_loop_resources.py does: no GPU, no recompilation."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = 'k_smoke_scatter_grad<0>'


@pytest.fixture(scope='module')
def kres():
    import __graft_entry__ as g
    g.build()                                                 # (up to date unless the sources changed)
    spec = importlib.util.spec_from_file_location('kres', os.path.join(ROOT, 'scripts', 'kres.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_scatter_kernel_uses_no_scratch(kres):
    res = kres.kernel_resources()
    assert KERNEL in res, 'kernel not found in the code object'
    r = res[KERNEL]
    assert r['scratch'] == 0 and r['vgpr_spills'] == 0, r
    assert r['vgpr'] <= 64, r                                 # one thread per distinct cell, a handful of words per lane
    assert r['lds'] == 0, r


def test_scatter_kernel_sits_behind_the_plain_kernels(kres):
    """a template instantiation is emitted behind every plain kernel: it does not come between two plain kernels of the parent, nor between
    two kernels of the 16 KB-aligned substep group"""
    addr = kres.kernel_addresses()
    first, last = addr[KERNEL][0], addr[KERNEL][0] + addr[KERNEL][1]
    for plain in ('k_render_shade', 'k_mesh_sdf', 'k_obs_gather', 'k_smoke_gather', 'k_smoke_loss_bwd', 'k_smoke_summary_merge', 'k_smoke_axpy'):
        assert addr[plain][0] < first, plain
    aligned = [addr[k][0] for k in ('k_p2g<true, false>', 'k_g2p_p2g<false>', 'k_pgg_g2pg<4, false>', 'k_grid<false, false, false>', 'k_g2p<false>',
                                    'k_g2p_grad2<4>', 'k_grid_grad<false, false>', 'k_p2g_grad<false, 4>')]
    assert all(a % 16384 == 0 for a in aligned), [hex(a) for a in aligned]
    assert last <= min(aligned) or first >= max(aligned), (hex(first), hex(last), [hex(v) for v in aligned])
