"""ClosedLoopSolver.forward_backward on Circulation-v0 against central differences of the rollout, on the fp64 oracle through the dense road
(CPU): the policy observes the smoke field, its cotangent goes back through CirculationEnv.obs_backward into the smoke frame's adjoint.

Scene: tests/test_host_env.py::_circulation (res 32, 10 Jacobi sweeps, its six detectors), horizon H below; the AirCon starts at the demo's
pose.  Policy: ObsPolicy(use_agent_state=False, hidden=16, input_gain=GAIN) in fp64; the bounds of CirculationEnv.action_bounds() leave it the
yaw rate (entry 4), strength and radius are the demo's.

The yardstick is tests/test_closed_loop_oracle.py's own: with FD_h and FD_h/2 the central differences at h = STEP and STEP / 2 along a unit
direction in parameter space, |adjoint - FD_h/2| <= 10 |FD_h - FD_h/2| + 1e-9 |FD_h/2|; the direct term alone (obs_backward skipped) must
miss that tolerance by more than 10 x in at least 3 of the 4 directions.  H, STEP and GAIN were chosen on the CPU so that the reference
meets both conditions (profiles/closed_loop_parity.txt section 4 has the table and the values that were tried):
  H = 6, STEP = 1e-4, GAIN = 10 (loss 3.3534; fp64 rounding of the difference quotient ~1e-11, the derivatives 1e-3 .. 3e-2)
  direction   FD_h/2               adjoint              |adj - FD|   tolerance   |direct - FD| / tolerance
  0            8.738359547067e-03   8.738359651070e-03  1.040e-10    2.496e-09   8,977
  1           -2.998287639500e-02  -2.998287637025e-02  2.475e-11    8.071e-10   111,619
  2            1.329771192271e-02   1.329771193915e-02  1.643e-11    1.687e-10   142,504
  3           -8.203945345286e-04  -8.203945191007e-04  1.543e-11    4.227e-10   1,770
At horizon 4 the observation adjoint is exactly zero (the yaw rate of step i reaches the field in step i + 1 and a detector later still: full
and direct gradients are the same bits), at 5 and 6 it is 3e-3 .. 4e-3 of the gradient; at STEP = 1e-3 the tolerance is 100 x wider and the
direct term misses it by 2 .. 7 x only; GAIN = 30 misses by 180 .. 690 x, GAIN = 100 by 10 .. 590 x, GAIN = 300 and above saturate the first layer.
Resident and chunked (max_substeps_local = two steps) gradients: relative L2 asserted <= 1e-12."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

from test_host_env import _circulation
from fluidlab_amd.optimizer.closed_loop import ClosedLoopSolver, ObsPolicy

H = 6
STEP = 1e-4                                                      # h of the central difference, along a unit direction
GAIN = 10.0
HIDDEN = 16
START_POSE = [0.55, 0.5, 0.27, 0.0, 0.0, 0.0, 0.0, 0.0]          # CirculationEnv.demo_policy's pose row


def build(lib, max_substeps_local, **kw):
    env = _circulation(lib, max_substeps_local=max_substeps_local, ckpt_dest='cpu', **kw)
    env.taichi_env.loss.temporal_range[1] = H
    pol = ObsPolicy(env, hidden=HIDDEN, use_agent_state=False, input_gain=GAIN, seed=1, actions_p=START_POSE)
    return env, pol, ClosedLoopSolver(env, pol)


@pytest.fixture(scope='module')
def resident(oracle64):
    env, pol, sol = build(oracle64, None)
    assert pol.dtype == torch.float64 and pol.device.type == 'cpu'
    state = env.taichi_env.get_state()['state']
    info = sol.forward_backward(state)
    g = sol.grad_vector()
    sol.skip_obs_backward = True
    sol.forward_backward(state)
    g_direct = sol.grad_vector()
    sol.skip_obs_backward = False
    return dict(env=env, pol=pol, sol=sol, state=state, g=g, g_direct=g_direct, loss=info['loss'])


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


def test_fixed_action_entries_carry_no_gradient_and_the_radius_stays_positive(resident):
    pol = resident['pol']
    o = resident['sol']._observe()
    a = pol(o).detach().numpy()
    assert (a[[0, 1, 2, 3, 5]] == 0).all() and a[6] == 0.02 and a[7] == 0.04 and abs(a[4]) <= 0.1


def test_chunked_sweep_equals_the_resident_one(resident, oracle64):
    ns = resident['env'].taichi_env.simulator.n_substeps
    env, pol, sol = build(oracle64, 2 * ns)                       # two steps per chunk: the sweep crosses a chunk boundary
    assert env.taichi_env.simulator.max_substeps_local == 2 * ns < H * ns
    pol.load_state_dict(resident['pol'].state_dict())
    info = sol.forward_backward(env.taichi_env.get_state()['state'])
    g = sol.grad_vector()
    rel = np.linalg.norm(g - resident['g']) / np.linalg.norm(resident['g'])
    print(f'chunked against resident: relative L2 {rel:.3e}, loss {info["loss"]!r} against {resident["loss"]!r}')
    assert info['loss'] == pytest.approx(resident['loss'], rel=1e-12)
    assert rel <= 1e-12
