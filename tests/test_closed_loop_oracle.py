"""ClosedLoopSolver.forward_backward against central differences of the rollout, on the fp64 oracle through the dense road (CPU).

Scene: Mixing-v0 at quality 0.5, particle density 3e4, horizon 4 (2,592 particles, 10 substeps per step): the stirrer starts inside the
coffee, so the tool touches the fluid from the first step and what the policy observes depends on what it did one step earlier.
Policy: ObsPolicy(use_agent_state=False, hidden=16, input_gain=30) in fp64.

The yardstick is the finite difference's own truncation: with FD_h and FD_h/2 the central differences at h = 1e-3 and 5e-4 along a unit
direction in parameter space, |adjoint - FD_h/2| <= 10 |FD_h - FD_h/2| + 1e-9 |FD_h/2|.  (h: the loss is 5.5e-3 and the directional
derivatives 1e-6, so fp64 rounding of the difference quotient is ~1e-12 of them; the first-layer weights are 0.016 at most and see the
input 30 times enlarged, and at h = 2e-2 a contact kink falls inside one direction's interval.)

Measured (four directions; profiles/closed_loop_parity.txt has the full figures):
  direction   FD_h/2               adjoint              |adj - FD|   tolerance   |direct - FD| / tolerance
  0           -7.414397333941e-07  -7.414401971522e-07  4.638e-13    1.006e-11   374,882
  1            1.919846232511e-06   1.919846964542e-06  7.320e-13    2.202e-11   48,277
  2            4.794735580793e-07   4.794736256819e-07  6.760e-14    2.052e-12   1,218,750
  3            1.179955892543e-06   1.179955738684e-06  1.539e-13    4.772e-12   217,479
The direct term alone (obs_backward skipped: sum_i J_pi^T dL/da_i) must miss the same tolerance by more than 10 x in at least 3 of the 4
directions -- without the observation adjoint the test fails; here it misses in all four.  Resident and chunked (max_substeps_local =
two steps) gradients: relative L2 0.0 measured, 1e-12 asserted (the oracle's replay of a chunk repeats its bits)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

from fluidlab_amd.envs import make
from fluidlab_amd.optimizer.closed_loop import ClosedLoopSolver, ObsPolicy

H = 4
STEP = 0.001                                                     # h of the central difference, along a unit direction


def _build(lib, max_substeps_local):
    env = make('Mixing-v0', seed=0, loss=True, engine_lib=lib, quality=0.5, particle_density=3e4, horizon=H,
               max_substeps_local=max_substeps_local, ckpt_dest='cpu')
    env.taichi_env.loss.temporal_range[1] = H
    pol = ObsPolicy(env, hidden=16, use_agent_state=False, input_gain=30.0, seed=1)
    assert pol.dtype == torch.float64 and pol.device.type == 'cpu'
    return env, pol, ClosedLoopSolver(env, pol)


@pytest.fixture(scope='module')
def resident(oracle64):
    env, pol, sol = _build(oracle64, None)
    state = env.taichi_env.get_state()['state']
    info = sol.forward_backward(state)
    g = sol.grad_vector()
    sol.skip_obs_backward = True
    sol.forward_backward(state)
    g_direct = sol.grad_vector()
    sol.skip_obs_backward = False
    return dict(env=env, pol=pol, sol=sol, state=state, g=g, g_direct=g_direct, loss=info['loss'])


def test_tool_touches_the_fluid_from_the_first_step(resident):
    """the scene condition: the stirrer's position lies inside the coffee body's bounding box at frame 0"""
    te = resident['env'].taichi_env
    pos = np.asarray(te.agent.get_state(0)[0][:3])
    x = np.asarray(resident['state']['x'])
    coffee = x[np.asarray(te.particles['body_id']) == 1]
    assert (coffee.min(axis=0) < pos).all() and (pos < coffee.max(axis=0)).all(), (pos, coffee.min(axis=0), coffee.max(axis=0))


def test_adjoint_matches_central_differences_and_the_direct_term_does_not(resident):
    pol, sol, state, g, g_direct = (resident[k] for k in ('pol', 'sol', 'state', 'g', 'g_direct'))
    params = list(pol.parameters())
    theta0 = torch.cat([p.detach().reshape(-1) for p in params]).clone()
    assert g.shape == (theta0.numel(),) and np.isfinite(g).all() and np.abs(g).max() > 0
    rng = np.random.RandomState(7)
    dirs = [rng.normal(size=theta0.numel()) for _ in range(4)]
    dirs = [d / np.linalg.norm(d) for d in dirs]

    def loss_at(theta):
        k = 0
        with torch.no_grad():
            for p in params:
                p.copy_(theta[k:k + p.numel()].reshape(p.shape)); k += p.numel()
        return sol.rollout(state)['loss']

    def central(d, h):
        dd = torch.as_tensor(d, dtype=theta0.dtype)
        return (loss_at(theta0 + h * dd) - loss_at(theta0 - h * dd)) / (2 * h)

    missed = 0
    try:
        for k, d in enumerate(dirs):
            f1, f2 = central(d, STEP), central(d, STEP / 2)
            adj, direct = float(g @ d), float(g_direct @ d)
            tol = 10 * abs(f1 - f2) + 1e-9 * abs(f2)
            print(f'direction {k}: FD_h {f1:.12e} FD_h/2 {f2:.12e} adjoint {adj:.12e} |adj - FD| {abs(adj - f2):.3e} tolerance {tol:.3e} '
                  f'direct term {direct:.12e} |direct - FD| / tolerance {abs(direct - f2) / tol:.1f}')
            assert abs(adj - f2) <= tol, (k, adj, f2, tol)
            missed += abs(direct - f2) >= 10 * tol
    finally:
        loss_at(theta0)
    assert missed >= 3, f'the direct term alone misses the tolerance by 10 x in only {missed} of 4 directions: the scene does not test the observation adjoint'


def test_chunked_sweep_equals_the_resident_one(resident, oracle64):
    ns = resident['env'].taichi_env.simulator.n_substeps
    env, pol, sol = _build(oracle64, 2 * ns)                      # two steps per chunk: the sweep crosses a chunk boundary
    assert env.taichi_env.simulator.max_substeps_local == 2 * ns < H * ns
    pol.load_state_dict(resident['pol'].state_dict())
    info = sol.forward_backward(env.taichi_env.get_state()['state'])
    g = sol.grad_vector()
    rel = np.linalg.norm(g - resident['g']) / np.linalg.norm(resident['g'])
    print(f'chunked against resident: relative L2 {rel:.3e}, loss {info["loss"]!r} against {resident["loss"]!r}')
    assert info['loss'] == pytest.approx(resident['loss'], rel=1e-12)
    assert rel <= 1e-12
