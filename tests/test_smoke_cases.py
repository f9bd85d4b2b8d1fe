"""The smoke solver's edge cases (tests/smoke_cases.py) on the CPU: the conditions the case table promises, the C++ oracle against the
numpy restatement stage by stage on every case, and finite differences of the oracle's hand-derived adjoint where the slab meets the
walls, with three temperature channels and in the pocket.  The oracle is the reference of test_smoke_hip_stages.py: it is pinned here
where it is used there."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import smoke_cases as SC  # noqa: E402
import smoke_numpy  # noqa: E402  (smoke_cases puts oracle/ on the path)


def test_smoke_case_table_conditions():
    """pocket: a free cell with no free neighbour, one with exactly one, and open space besides; every static: no cell centre within
    1e-3 voxels of its surface (an fp32 and an fp64 sample agree on every cell); fast cases: the step-0 back-trace leaves the grid
    through each of its six faces."""
    for name in ('pocket', 'fast-pocket'):
        free = SC.free_mask(SC.CASES[name])
        nb = SC.free_neighbours(free)
        assert free[SC.POCKET_ISOLATED] and nb[SC.POCKET_ISOLATED] == 0
        assert free[SC.POCKET_DEAD_END] and nb[SC.POCKET_DEAD_END] == 1 and all(free[c] and nb[c] == 1 for c in SC.POCKET_PAIR)
        assert (free & (nb == 0)).sum() == 1 and (free & (nb == 1)).sum() >= 3
        assert (free & (nb >= 2)).sum() > 100
    for name in SC.NAMES:
        case = SC.CASES[name]
        for sd, lip in SC.static_sdf_at_centres(case):
            assert np.abs(sd).min() > 1e-3 * max(lip, 1.0), (name, np.abs(sd).min(), lip)   # |sdf| > 1e-3 L: no zero within 1e-3 voxels
        free = SC.free_mask(case)
        j = np.arange(case['res'])
        slab = (j > case['ly']) & (j < case['hy'])
        assert not free[:, ~slab].any()
        if case['statics'] != 'none':
            assert 0 < (~free[:, slab]).sum() < free[:, slab].size, name               # the statics take cells out of the slab
        else:
            assert free[:, slab].all()
    two = SC.free_mask(SC.CASES['q2-one-sweep'])
    assert (~two[0, 4:8]).any()                                                          # the second static reaches the x = 0 wall
    assert SC.free_mask(SC.CASES['empty']).sum() == 0 and SC.free_mask(SC.CASES['one-layer']).sum() == 12 * 12
    for name in SC.FAST:
        case = SC.CASES[name]
        n = case['res']
        free = SC.free_mask(case)
        v0 = SC.inputs(case)[0]
        cells = np.argwhere(free)
        pb = smoke_numpy.backtrace(free, v0, cells + 0.5, SC.DT)
        for ax in range(3):
            assert (pb[:, ax] < 0).any() and (pb[:, ax] > n).any(), (name, ax)
        assert (np.abs(pb - (cells + 0.5)).max(1) > 2.0).mean() > 0.25                 # several cells, not half a cell


@pytest.mark.parametrize('name', SC.NAMES)
def test_smoke_case_oracle_matches_numpy(oracle64, name):
    """the fp64 oracle against oracle/smoke_numpy.py on all five fields over two steps (the bound of
    test_smoke_step_matches_numpy_restatement), with the numpy step taken stage by stage"""
    case = SC.CASES[name]
    free = SC.free_mask(case)
    eng, e = SC.make_engine(oracle64, case, action_steps=2)
    v, q, p = SC.inputs(case)
    acts = SC.actions(2)
    for s in range(2):
        eng.eff_set_action(e, s, s, 2, acts[s])
        eng.smoke_step(s, 2 * s)
        air = SC.aircon_at(eng, e, 2 * s)
        v_tmp, q = smoke_numpy.advect(v, q, free, SC.DT, air)
        div = smoke_numpy.divergence(v_tmp, free)
        p = smoke_numpy.jacobi(p, div, free, case['iters'])
        v = smoke_numpy.subtract(v_tmp, p, free)
        got0 = eng.smoke_get_frame(s, ('v_tmp', 'div'))
        got1 = eng.smoke_get_frame(s + 1, ('v', 'q', 'p'))
        assert ((got0['v_tmp'] != 0).any(-1) == free).all(), (s, 'free mask')
        for fname, ref, got in (('v_tmp', v_tmp, got0['v_tmp']), ('div', div, got0['div']), ('v', v, got1['v']), ('q', q, got1['q']), ('p', p, got1['p'])):
            assert np.abs(got - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), (s, fname, np.abs(got - ref).max())
        eng.step(2 * s, 2 * s, 2, 1)
    eng.close()


def _fd(run, exact, steps=(1e-4, 1e-5, 1e-6)):
    errs = []
    for h in steps:
        d = (run(+h) - run(-h)) / (2 * h)
        errs.append(abs(d - exact) / max(abs(d), 1e-6))
    return min(errs)


def _cells_for(name, free):
    """cells to perturb: next to a domain wall, next to an obstacle, and (pocket) the cavities"""
    nb = SC.free_neighbours(free)
    n = free.shape[0]
    I = np.indices(free.shape)
    at_domain_wall = free & ((I == 0) | (I == n - 1)).any(0)
    at_obstacle = free & (nb < 6) & ~at_domain_wall & (nb >= 2)
    cells = [tuple(np.argwhere(at_domain_wall)[len(np.argwhere(at_domain_wall)) // 3]), tuple(np.argwhere(at_obstacle)[len(np.argwhere(at_obstacle)) // 2])]
    if name == 'pocket':
        cells += [SC.POCKET_ISOLATED, SC.POCKET_PAIR[0], SC.POCKET_DEAD_END]
    return cells


@pytest.mark.parametrize('name', ['q3', 'walls', 'pocket'])
def test_smoke_case_adjoint_vs_finite_differences(oracle64, name):
    """test_smoke_adjoint_vs_finite_differences (same method, same 1e-5 bound) on the cases whose adjoint the HIP parity tests lean on:
    an action component of each kind, and the velocity and temperature of cells at a domain wall, at an obstacle and in the pocket."""
    case = SC.CASES[name]
    n, H = case['res'], 3
    free = SC.free_mask(case)
    rng = np.random.RandomState(3)
    cot_v, cot_q = rng.normal(size=(n, n, n, 3)), rng.normal(size=(n, n, n, case['q_dim']))
    acts = SC.actions(H)
    out = SC.run_steps(oracle64, case, acts, cot_v, cot_q)
    g = out['action_grad']
    assert np.abs(g[:, 6]).min() > 1e-6 and np.abs(g[:, 7]).min() > 1e-6 and np.abs(g[:, :3]).max() > 1e-6 and np.abs(g[:, 3:6]).max() > 1e-6
    for s_, k_ in [(0, 1), (1, 4), (2, 6), (0, 7)]:                                    # translation, rotation, strength, radius
        def run(dh, s_=s_, k_=k_):
            a = acts.copy(); a[s_, k_] += dh
            return SC.run_steps(oracle64, case, a, cot_v, cot_q)['loss']
        assert _fd(run, g[s_, k_]) < 1e-5, (name, 'action', s_, k_)
    qd = case['q_dim']
    for ci, cell in enumerate(_cells_for(name, free)):
        for field, comp, exact in (('v', ci % 3, out['gv0'][cell][ci % 3]), ('q', ci % qd, out['gq0'][cell][ci % qd])):
            def run(dh, field=field, idx=cell + (comp,)):
                return SC.run_steps(oracle64, case, acts, cot_v, cot_q, perturb=(field, idx, dh))['loss']
            assert _fd(run, exact) < 1e-5, (name, field, cell, comp)
