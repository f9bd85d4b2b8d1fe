"""GPU: the closed loop with a field observation on the MI355X.  Scene and policy of tests/test_closed_loop_fields_oracle.py (Mixing-v0,
quality 0.5, particle density 3e4, horizon 4, coffee on 16 x 1 x 16 with four channels, no particle rows, input_gain 300).

The yardstick is the one of tests/test_closed_loop_hip.py and the rigid-body tests: the fp32 oracle's relative-L2 distance from the fp64
oracle's parameter gradient, computed here.  The device road (fe_field_obs_get_dev / fe_field_obs_add_grad_dev, nothing downloaded) must lie
within twice that distance of the fp64 oracle's gradient, and the device road and the dense host road (downloaded frame, interpreter,
add_grad) on the same engine within that distance (once, not twice) of each other.

Measured (profiles/closed_loop_parity.txt section 5): fp32 oracle against fp64 oracle 2.469e-04; device road against fp64 3.078e-04 (1.247 x),
dense host road against fp64 3.166e-04, device road against dense host road 1.803e-05 (0.073 x).  fe_get_frame calls by ObsPolicy's o_0 / by one
_observe(): 0 / 0 on the device road, 2 / 2 on the host road."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import scenarios as S
from fluidlab_amd import _capi
from test_closed_loop_fields_oracle import build

pytestmark = pytest.mark.gpu


def _loop(lib, device_obs, count=None):
    at = {}
    env, pol, sol = build(lib, None, device_obs, before_policy=(lambda: at.update(n=count['n'])) if count is not None else None)
    assert sol._device_road() == bool(device_obs)
    if count is not None:                                         # downloads since the environment stood: by ObsPolicy's o_0, then by one _observe
        count['policy'] = count['n'] - at['n']
        sol._observe()
        count['observe'] = count['n'] - at['n'] - count['policy']
    info = sol.forward_backward(env.taichi_env.get_state()['state'])
    g = sol.grad_vector()
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    return g, info['loss']


@pytest.fixture(scope='module')
def oracles(oracle32, oracle64):
    g64, l64 = _loop(oracle64, False)
    g32, l32 = _loop(oracle32, False)
    return g64, g32, l64, l32


def test_device_road_against_the_fp64_oracle_and_the_dense_road(hiplib, oracles, monkeypatch):
    g64, g32, l64, l32 = oracles
    yard = S.rel_l2(g32, g64)
    count = {'n': 0}
    real = _capi.Engine.get_frame

    def counting(self, *a, **k):
        count['n'] += 1
        return real(self, *a, **k)

    monkeypatch.setattr(_capi.Engine, 'get_frame', counting)
    count['n'] = 0
    gd, ld = _loop(hiplib, True, count)
    n_dev = dict(count)
    count['n'] = 0
    gh, lh = _loop(hiplib, False, count)
    n_host = dict(count)
    rel_dev, rel_host, rel_roads = S.rel_l2(gd, g64), S.rel_l2(gh, g64), S.rel_l2(gd, gh)
    print(f'closed loop with a field observation: fp32 oracle against fp64 oracle {yard!r}; HIP device road against fp64 {rel_dev!r} ({rel_dev / yard:.3f} x), '
          f'HIP dense host road against fp64 {rel_host!r}, device road against dense road {rel_roads!r} ({rel_roads / yard:.3f} x); '
          f'losses fp64 {l64!r} fp32 oracle {l32!r} HIP device {ld!r} HIP dense {lh!r}; fe_get_frame calls: device road {n_dev}, host road {n_host}')
    assert yard > 0
    assert rel_dev <= 2 * yard, (rel_dev, yard)
    assert rel_roads <= yard, (rel_roads, yard)
    # ObsPolicy (its o_0) and _observe download no frame on the device road; the host road does
    assert n_dev['policy'] == 0 and n_dev['observe'] == 0, n_dev
    assert n_host['policy'] > 0 and n_host['observe'] > 0, n_host


def test_particle_rows_and_fields_together_on_the_device_road(hiplib):
    """what `run.py --closed_loop --field_obs N` sets up: enable_device_obs() and enable_field_obs(..., particles=True).  The tensor _observe()
    assembles on the GPU is the vector _get_obs() builds, word for word in the order of obs_layout(), and obs_backward() routes a cotangent
    that lives on the GPU -- particle rows, pose and field block -- to the bits the same cotangent gives from the host"""
    import torch
    from fluidlab_amd.envs import make
    from fluidlab_amd.optimizer.closed_loop import ClosedLoopSolver, ObsPolicy
    from test_closed_loop_fields_oracle import FIELDS, H
    env = make('Mixing-v0', seed=0, loss=True, engine_lib=hiplib, quality=0.5, particle_density=3e4, horizon=H, max_substeps_local=None, ckpt_dest='cpu')
    env.enable_device_obs()
    env.enable_field_obs(FIELDS, particles=True)
    pol = ObsPolicy(env, hidden=16, use_agent_state=True, seed=1)
    sol = ClosedLoopSolver(env, pol)
    assert sol._device_road()
    te = env.taichi_env
    te.set_state(te.get_state()['state'], grad_enabled=True)
    te.step(np.zeros(te.agent.action_dim))                        # a frame with velocities
    layout = env.obs_layout()
    assert layout['bodies'] and layout['agent'] and len(layout['fields']) == 1 and layout['fields'][0]['slice'].stop == layout['size']
    with torch.no_grad():
        o_dev = sol._observe()
    o_host = np.asarray(env._get_obs())
    assert o_dev.is_cuda and tuple(o_dev.shape) == o_host.shape == (layout['size'],)
    got, want = o_dev.cpu().numpy(), o_host.astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    blk = got[layout['fields'][0]['slice']].reshape(layout['fields'][0]['shape'])
    assert blk[0].sum() > 2000 and np.abs(blk[1:]).max() > 0 and np.abs(got[layout['bodies'][0]['v']]).max() > 0
    # the cotangent: from the GPU and from the host
    eng = te.simulator.engine
    f = te.simulator.cur_substep_local
    g = np.random.RandomState(3).normal(size=layout['size']).astype(np.float32)
    out = []
    for cot in (torch.as_tensor(g, device=pol.device), g):
        eng.reset_grad()
        for e in te.agent.effectors:
            assert not eng.eff_get_state_grad(e.index, f).any()
        env.obs_backward(cot, f=f)
        out.append(list(eng.get_grad(f)) + [eng.eff_get_state_grad(e.index, f) for e in te.agent.effectors])
    for a, b in zip(*out):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    gx, gv = out[0][:2]
    ids = np.concatenate([b['ids'] for b in layout['bodies']])
    listed = np.zeros(eng.N, bool); listed[ids] = True
    coffee = np.asarray(te.simulator._mat_np) == FIELDS[0]['mat']
    assert np.abs(gx[coffee & ~listed]).max() > 0 and np.abs(gv[coffee & ~listed]).max() > 0      # the field's share: particles no row names
    assert np.abs(gx[listed & ~coffee]).max() > 0 and not gx[~listed & ~coffee].any()              # the rows' share: milk the field does not select
    assert all(np.abs(p).max() > 0 for p in out[0][4:])
    eng.reset_grad()
