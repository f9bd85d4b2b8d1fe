"""The kernels of a substep pair take their head arguments preloaded in SGPRs (fe_engine.hip "kernel heads"): what each kernel's first
loads ask with leads its signature as plain pointers and ints, and the build switches kernarg preloading on.  Preloading stops at the
first aggregate and at 14 dwords, so a struct moved to the front, a head that outgrew the budget or a build without the flag shows as a
preload length below the head's size.  Reads the kernel descriptors of the code object inside the built libfluidengine_hip.so
(scripts/kres.py kernel_preload): no GPU, no recompilation."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# dwords of the head arguments, from the signatures in fe_engine.hip (a pointer is two, an int one)
UNITS = 2 + 2 + 1                   # (h_units | h_units_p | h_list, h_meta, h_cap)
UNITS_2 = 2 + 2 + 2 + 1             # (h_units, h_units_p, h_meta, h_cap)
GRID = 6 * 2 + 2                    # (h_active, h_touched, h_dirty, h_nbr, h_meta, blk_count, nb3, n_wg)
GRID_GRAD = 5 * 2 + 4               # (h_active, h_live, h_dirty, h_nbr, h_meta, nb3, n_wg, h_cap, h_stored)
# the liquid-only and the general (SVD) instantiations a substep pair launches with the default options, the recompute of a frame
# whose grid was not stored, and the g2p of a frame the order is rebuilt on
HEAD_DWORDS = {
    'k_p2g<true, false>': UNITS, 'k_p2g<true, true>': UNITS, 'k_p2g<false, false>': UNITS, 'k_p2g<false, true>': UNITS,
    'k_g2p_p2g<false>': UNITS, 'k_g2p_p2g<true>': UNITS,
    'k_g2p<false>': UNITS, 'k_g2p<true>': UNITS, 'k_g2p_sortkey<false>': UNITS, 'k_g2p_sortkey<true>': UNITS,
    'k_g2p_grad2<4>': UNITS, 'k_g2p_grad2<3>': UNITS,
    'k_p2g_grad<false, 4>': UNITS_2, 'k_p2g_grad<true, 1>': UNITS_2,
    'k_pgg_g2pg<4, false>': UNITS, 'k_pgg_g2pg<3, true>': UNITS,
    'k_grid<false, false, false>': GRID, 'k_grid<true, false, false>': GRID, 'k_grid<false, true, false>': GRID,
    'k_grid_grad<false, false>': GRID_GRAD, 'k_grid_grad<true, false>': GRID_GRAD,
}
BUDGET = 14                         # 16 user SGPRs less the address of the argument segment


@pytest.fixture(scope='module')
def preload():
    import __graft_entry__ as g
    g.build()                                                 # (up to date unless the sources changed)
    spec = importlib.util.spec_from_file_location('kres', os.path.join(ROOT, 'scripts', 'kres.py'))
    kres = importlib.util.module_from_spec(spec); spec.loader.exec_module(kres)
    return kres.kernel_preload()


def test_heads_fit_the_preload_budget():
    over = {k: n for k, n in HEAD_DWORDS.items() if n > BUDGET}
    assert not over, over


def test_substep_kernels_preload_their_heads(preload):
    missing = [k for k in HEAD_DWORDS if k not in preload]
    assert not missing, f'kernels not found in the code object: {missing} (have: {sorted(preload)[:8]} ...)'
    short = {k: (preload[k], n) for k, n in HEAD_DWORDS.items() if preload[k] < n}
    assert not short, f'head arguments not preloaded (preload length, head dwords): {short}'


def test_batched_entry_points_take_one_struct(preload):
    """The other side of the reading: a kernel whose first argument is an aggregate preloads nothing, so the descriptor field read above is
    the one that tells the two apart."""
    for k in ('k_grid_b<false, false, false>', 'k_g2p_p2g_b<false>', 'k_pgg_g2pg_b<4>'):
        assert preload[k] == 0, (k, preload[k])
