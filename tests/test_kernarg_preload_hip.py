"""GPU: the substep kernels read their unit lists, the active list, the marks and the list lengths through head arguments that arrive
preloaded in SGPRs (fe_engine.hip "kernel heads"), and the same words travel a second time inside TableP / GridStore for everything
behind the head.  A head argument that disagrees with its struct twin -- the wrong list, another table's meta, a stale row of the live
marks, a workgroup count that is not the launch's -- is a wrong trajectory or a wrong adjoint, far outside fp32 noise."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402

pytestmark = pytest.mark.gpu

# What the call sequence below launches (profile_read), as the engine launched it before the heads existed: the structure has not moved.
# 13 substeps, an order rebuilt at 0, 4, 8, 12, two fe_step calls (0-5, 6-12): a fused g2p_p2g wherever the substep before belongs to the
# same call and no sort lies between (1 2 3 5 | 7 9 10 11), p2g at the sorts and at the head of the second call (0 4 | 6 8 12), a separate
# g2p in front of every sort and at the end of a call (3 5 | 7 11 12) -- the ones at 3, 7 and 11 leave the sort's keys (no sort_count for
# 4, 8, 12).  The reverse sweep is one call over stored grids (no recompute): p2g_grad takes the g2p_grad of the substep before along where
# both share an order (pgg_g2pg at 1 2 3 5 6 7 9 10 11), alone at 0 4 8 12, g2p_grad alone at 12 11 7 3.
LAUNCHES = {'p2g': 5, 'g2p_p2g': 8, 'g2p': 5, 'grid_op': 13, 'p2g_recompute': 0, 'grid_op_keep': 0,
            'g2p_grad': 4, 'grid_op_grad': 13, 'p2g_grad': 4, 'pgg_g2pg': 9, 'sort': 4}


def test_head_arguments_agree_with_their_struct_twins(hiplib, oracle64):
    """The 32^3 / 6,000-particle block of test_fused_g2p_p2g_launch_matches_separate_launches (random velocities, a tenth of the slots
    unused, sort_interval 4) with the default options: pair units, tail units, a sort boundary inside and between the calls, the separate
    and the fused kernels of both sweeps.  Against the fp64 oracle with that test's bounds for its oracle comparison."""
    rng = np.random.RandomState(5)
    N, n_sub = 6000, 13
    sc = S.water_block(n_grid=32, n_particles=N, seed=3, lo=0.3, hi=0.6)
    sc['v'] = S.f32(rng.normal(0, 1.0, (N, 3)) + [2.0, -3.0, 1.0])
    sc['used'] = (rng.rand(N) > 0.1).astype(np.int32)
    cot = S.random_cotangent(N, seed=7)

    def run(lib, opts, ranged):
        g = S.make_engine(lib, sc, options=opts)
        if lib is hiplib:
            g.profile_enable(True)
        if ranged:
            g.step(0, 0, 6, 0)
            g.step(6, 6, n_sub - 6, 0)
        else:
            for f in range(n_sub):
                g.substep(f, f, 0)
        last = S.get_state(g, n_sub)
        g.reset_grad()
        g.add_grad(n_sub, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
        g.step_grad(0, 0, n_sub, 0)
        grad = dict(zip(('gx', 'gv', 'gC', 'gF'), g.get_grad(0)))
        prof = g.profile_read() if lib is hiplib else None
        g.close()
        return last, grad, prof

    a, ga, prof = run(hiplib, {'sort_interval': 4}, True)
    o, go, _ = run(oracle64, {}, False)
    launches = {k: int(prof[k][1]) for k in LAUNCHES}
    print('MEASURED kernel heads: launches', launches, '| vs fp64 oracle x', np.abs(a['x'] - o['x']).max(), 'v', S.rel_l2(a['v'], o['v']),
          {k: round(S.rel_l2(ga[k], go[k]), 8) for k in ga})
    assert launches == LAUNCHES, launches
    assert (a['used'] == o['used']).all()
    assert np.abs(a['x'] - o['x']).max() <= 5e-6 and S.rel_l2(a['v'], o['v']) <= 1e-3
    for k in ('gx', 'gv', 'gC', 'gF'):
        assert np.isfinite(ga[k]).all()
        assert S.cosine(ga[k], go[k]) >= 0.999 and S.rel_l2(ga[k], go[k]) <= 3e-3, (k, S.rel_l2(ga[k], go[k]))
