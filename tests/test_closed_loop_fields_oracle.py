"""ClosedLoopSolver.forward_backward with a FIELD observation against central differences of the rollout, on the fp64 oracle through the
host road (CPU): the frame is downloaded, term_program.field_obs_of_points builds the observation and field_obs_grad_of_points + add_grad
carry its cotangent back.

Scene: that of tests/test_closed_loop_oracle.py -- Mixing-v0 at quality 0.5, particle density 3e4, horizon 4 (2,592 particles, 10 substeps
per step), ObsPolicy(hidden=16, use_agent_state=False) in fp64.  Observation: enable_field_obs([coffee: 16 x 1 x 16 over the cup's box,
channels 4], particles=False): 1,024 values behind the (masked) pose, no particle row.

The yardstick is that test's: with FD_h and FD_h/2 the central differences at h = 1e-3 and 5e-4 along a unit direction in parameter space,
|adjoint - FD_h/2| <= 10 |FD_h - FD_h/2| + 1e-9 |FD_h/2|.  The direct term alone (obs_backward skipped) must miss that tolerance by more than
10 x in at least 3 of the 4 directions: without the routing of the field slices the test fails.

input_gain is 300, not that test's 30.  A field block is divided by its largest density value (about 20 particles per cell), and over four
steps a cell's content changes by hundredths of that: at gain 30 and at gain 100 the adjoint met the tolerance in all four directions but
the direct term missed it by 10 x in only two of them (5.3 x and 3.0 x, 8.0 x and 2.7 x in the other two) -- the scene did not test the
field adjoint.  The margin stayed; the gain went up.

Measured at gain 300 (profiles/closed_loop_parity.txt has the other gains):
  direction   FD_h/2               adjoint              |adj - FD|   tolerance   |direct - FD| / tolerance
  0            8.554374414556e-06   8.554336726227e-06  3.769e-11    2.696e-09   105.0
  1           -5.353482187068e-06  -5.353711122188e-06  2.289e-10    1.204e-09   722.6
  2           -5.941180070482e-06  -5.941113498394e-06  6.657e-11    1.368e-10   1233.9
  3            7.717167354801e-06   7.717286744155e-06  1.194e-10    1.661e-09   482.6
Resident and chunked (max_substeps_local = two steps) gradients: relative L2 0.0 measured, 1e-12 asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

from fluidlab_amd.configs.macros import COFFEE_VIS
from fluidlab_amd.envs import make
from fluidlab_amd.optimizer.closed_loop import ClosedLoopSolver, ObsPolicy

H = 4
STEP = 0.001
GAIN = 300.0
FIELDS = [dict(lower=(0.08, 0.4, 0.08), upper=(0.92, 0.95, 0.92), n=(16, 1, 16), mat=COFFEE_VIS, channels=4)]


def build(lib, max_substeps_local=None, device_obs=False, before_policy=None):
    env = make('Mixing-v0', seed=0, loss=True, engine_lib=lib, quality=0.5, particle_density=3e4, horizon=H,
               max_substeps_local=max_substeps_local, ckpt_dest='cpu')
    env.taichi_env.loss.temporal_range[1] = H
    if device_obs:
        env.enable_device_obs()
    env.enable_field_obs(FIELDS, particles=False)
    if before_policy is not None:
        before_policy()
    pol = ObsPolicy(env, hidden=16, use_agent_state=False, input_gain=GAIN, seed=1)
    return env, pol, ClosedLoopSolver(env, pol)


@pytest.fixture(scope='module')
def resident(oracle64):
    env, pol, sol = build(oracle64)
    assert pol.dtype == torch.float64 and pol.device.type == 'cpu'
    state = env.taichi_env.get_state()['state']
    info = sol.forward_backward(state)
    g = sol.grad_vector()
    sol.skip_obs_backward = True
    sol.forward_backward(state)
    g_direct = sol.grad_vector()
    sol.skip_obs_backward = False
    return dict(env=env, pol=pol, sol=sol, state=state, g=g, g_direct=g_direct, loss=info['loss'])


def test_the_observation_is_the_field_alone(resident):
    env = resident['env']
    layout = env.obs_layout()
    n_pose = sum(s.stop - s.start for s in layout['agent'])
    assert layout['bodies'] == [] and len(layout['fields']) == 1 and layout['fields'][0]['shape'] == (4, 16, 1, 16) and layout['fields'][0]['channels'] == 4
    assert layout['size'] == n_pose + 1024 and layout['fields'][0]['slice'] == slice(n_pose, n_pose + 1024)
    o = env._get_obs()
    blk = o[layout['fields'][0]['slice']].reshape(4, 16, 1, 16)
    te = env.taichi_env
    n_coffee = int((np.asarray(te.simulator._mat_np) == COFFEE_VIS).sum())
    assert 0.97 * n_coffee <= blk[0].sum() <= n_coffee            # the coffee fills the cup to its wall: the outermost stencils reach over the box's edge
    assert np.abs(blk[1:]).max() == 0 or np.abs(blk[1:]).max() < 1e3
    pol = resident['pol']
    gain = pol.gain.numpy()[layout['fields'][0]['slice']]
    assert np.all(gain == GAIN / blk[0].max())                    # one constant per block, the largest density value of o_0


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
    assert missed >= 3, f'the direct term alone misses the tolerance by 10 x in only {missed} of 4 directions: the scene does not test the field adjoint'


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
