"""Non-finite velocities in a smoke frame are values, not addresses: the defined-behaviour statement of fe_smoke_index.h on the whole solver.

A 16^3 smoke engine with two Jacobi sweeps; frame 0's v holds +inf, -inf, NaN and 3e38, each at one free cell.  One fe_smoke_step and one
fe_smoke_step_grad run, every call and fe_sync return 0, and the field summary counts the non-finite cells of the frame that holds them.
The same through the environment: CirculationEnv.step() with enable_diagnostics() ends the episode, ClosedLoopSolver(check_finite=True)
raises FloatingPointError.
What the next frame holds is not asserted.  Measured on the MI355X: 0 non-finite cells of 1,024 in frame 1 -- a cell whose back-trace meets
a non-finite velocity gets a non-finite position, the index clamps it to the grid's edge with f = 0, and the sample there is finite; the
fp32 oracle, whose index is the old expression, leaves 379 cells of this scene non-finite instead.  That is why the environment's
diagnostics and the solver's check also look at the frame a step consumed.
(tests/test_smoke_index_hip.py checks the index itself, lane by lane, without touching memory: it comes first.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import test_host_env as H  # noqa: E402
import test_smoke as TS  # noqa: E402
from fluidlab_amd.optimizer.closed_loop import ClosedLoopSolver, ObsPolicy  # noqa: E402

pytestmark = pytest.mark.gpu

BAD = [np.inf, -np.inf, np.nan, 3e38]


def test_step_and_step_grad_with_nonfinite_velocities(hiplib):
    res = 16
    eng, e = TS.make_smoke_engine(hiplib, res=res, steps=2, solver_iters=2, obstacle=False)
    lib, h = eng.lib, eng.h
    v = eng.smoke_get_frame(0, ('v',))['v']
    cells = [(3, 5, 4), (8, 4, 11), (12, 6, 7), (6, 7, 13)]                  # inside the free slab 3 < j < 8, no obstacle
    for (i, j, k), bad in zip(cells, BAD):
        v[i, j, k, :] = [bad, 0.5, -bad if np.isfinite(bad) else bad]
    eng.smoke_set_frame(0, v=v)
    eng.eff_set_action(e, 0, 0, 2, TS._actions(1)[0])
    assert lib.fe_smoke_step(h, 0, 0) == 0
    assert lib.fe_sync(h) == 0
    rec = eng.smoke_summary(0)
    assert rec['n_nonfinite'] == 3 > 0 and rec['n_cells'] == res * 4 * res    # (+inf, -inf, NaN; 3e38 is finite, its back-trace is not representable as an index)
    nxt = eng.smoke_summary(1)
    print(f'non-finite cells: frame 0 {rec["n_nonfinite"]}, frame 1 {nxt["n_nonfinite"]} of {nxt["n_cells"]}')
    assert nxt['n_cells'] == res * 4 * res                                    # (how many of them are non-finite is not a contract: see the docstring)
    eng.reset_grad()
    n = res
    rng = np.random.RandomState(2)
    eng.smoke_add_grad(1, gv=rng.normal(size=(n, n, n, 3)).astype(np.float32), gq=rng.normal(size=(n, n, n, 1)).astype(np.float32))
    assert lib.fe_smoke_step_grad(h, 0, 0) == 0
    assert lib.fe_sync(h) == 0
    gv, gq = eng.smoke_get_grad(0)                                           # readable: whatever its values, it is memory of the frame
    assert gv.shape == (n, n, n, 3) and gq.shape == (n, n, n, 1)
    eng.close()


def test_the_environment_and_the_solver_stop_on_a_nonfinite_field(hiplib):
    env = H._circulation(None, max_substeps_local=None)
    env.enable_device_obs()
    env.enable_diagnostics()
    te = env.taichi_env
    sf = te.smoke_field
    state = te.get_state()['state']
    v = np.array(state['smoke_field']['v'])
    j = sf.lower_y + 1
    for (i, k), bad in zip([(5, 12), (12, 20), (20, 9), (27, 15)], BAD):
        v[i, j, k, 0] = bad
    state['smoke_field'] = dict(state['smoke_field'], v=v)
    te.set_state(state)
    assert te.smoke_summary()['n_nonfinite'] == 3
    obs, reward, done, info = env.step(np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.02, 0.04]))
    assert done and reward == -1000 and info['n_nonfinite'] > 0
    assert te.simulator.engine.lib.fe_sync(te.simulator.engine.h) == 0
    env.reset()
    pol = ObsPolicy(env, hidden=8, use_agent_state=False, seed=1)
    with pytest.raises(FloatingPointError):
        ClosedLoopSolver(env, pol, check_finite=True).rollout(state)
    assert te.simulator.engine.lib.fe_sync(te.simulator.engine.h) == 0
    info = ClosedLoopSolver(env, pol, check_finite=True).rollout(env._init_state['state'])     # a finite rollout passes the check
    assert np.isfinite(info['loss'])
