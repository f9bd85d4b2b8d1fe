"""The closed loop on Circulation-v0, what can be checked without a GPU: the new exports are in the header and in the cross-compiled library;
CirculationEnv.obs_layout() tiles the vector _get_obs() builds; action_bounds() of every registered environment -- the scalar range everywhere
but on Circulation, whose seven fixed entries come out of ObsPolicy exactly as the demo's row and whose radius cannot be commanded <= 0."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import test_host_env as H
from fluidlab_amd import _capi
from fluidlab_amd.envs import REGISTRY, make
from fluidlab_amd.optimizer.closed_loop import ObsPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['fe_smoke_obs_get', 'fe_smoke_obs_get_dev', 'fe_smoke_obs_add_grad', 'fe_smoke_obs_add_grad_dev', 'fe_eff_add_sr_grad', 'fe_eff_get_sr_grad']
DEMO_ROW = np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.02, 0.04])
FIXED = [0, 1, 2, 3, 5, 6, 7]


def test_new_exports_are_in_the_header_and_in_the_library():
    with open(os.path.join(ROOT, 'include', 'fluidengine_ext.h')) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r'extern int %s\(FeEngine\* h' % name, header), name
        assert name in _capi.EXT_SYMBOLS
    import __graft_entry__ as entry
    entry.build()                                                # (cross-compiles for gfx950 without a GPU; up to date after the first call)
    import ctypes
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, '__graft_entry__.py')) as f:
        assert "'fe_smoke_index.h'" in f.read()                  # the source hash sees the new header


def _small_env(name, lib):
    if name == 'Circulation-v0':
        return H._circulation(lib, max_substeps_local=None)
    if name == 'WaterBlock-v0':
        return make(name, quality=0.5, n_particles=4096, horizon=3, engine_lib=lib)
    if name == 'LatteArt-v0':
        return H._small(name, lib, loss=False, horizon=4, horizon_action=4, n_pool=300)
    if name == 'IceCreamDynamic-v0':
        return H._icecream(lib, loss=False, max_substeps_local=None)
    if name == 'LatteArtStir-v0':
        return H._stir(lib, loss=False, max_substeps_local=None)
    if name == 'IceCreamStatic-v0':
        return H._icecream_static(lib, loss=False, max_substeps_local=None)
    if name == 'GatheringEasy-v0':
        return H._gathering(lib)
    return H._small(name, lib, horizon=4)


@pytest.fixture(scope='module')
def circulation(oracle64):
    return H._circulation(oracle64, max_substeps_local=None)


def test_obs_layout_tiles_the_observation(circulation):
    env = circulation
    lay, obs = env.obs_layout(), env._get_obs()
    assert lay['size'] == len(obs) and lay['bodies'] == []
    sm = lay['smoke']
    n = len(sm['cells'])
    pieces = [lay['agent'][0], lay['extra'][0], sm['v'], sm['q']]
    at = 0
    for s in pieces:                                             # in order, without gaps or overlap
        assert s.start == at and s.stop > s.start
        at = s.stop
    assert at == lay['size']
    assert (lay['agent'][0].stop - lay['agent'][0].start, lay['extra'][0].stop - lay['extra'][0].start) == (7, 2)
    assert sm['v'].stop - sm['v'].start == 3 * n and sm['q'].stop - sm['q'].start == n * env.taichi_env.smoke_field.q_dim
    assert sm['list'] == env.OBS_LIST and sm['cells'].shape == (n, 3)
    # the rows are the lattice's cells in the order of the vector
    te = env.taichi_env
    env.step(DEMO_ROW); env.step(DEMO_ROW)
    obs = env._get_obs()
    st = te.smoke_field.get_state(te.simulator.cur_step_local)
    c = sm['cells']
    assert np.abs(st['v']).max() > 0
    assert (obs[sm['v']].reshape(n, 3) == st['v'][c[:, 0], c[:, 1], c[:, 2]]).all()
    assert (obs[sm['q']].reshape(n, -1) == st['q'][c[:, 0], c[:, 1], c[:, 2]]).all()
    env.reset()


def test_obs_backward_refuses_a_pose_cotangent_on_an_engine_without_the_extension(circulation):
    env = circulation
    lay = env.obs_layout()
    g = np.zeros(lay['size'])
    g[lay['smoke']['q']] = 1.0
    env.taichi_env.reset_grad()
    env.obs_backward(g, f=0)                                     # field rows alone: the dense road, every engine has it
    gv, gq = env.taichi_env.simulator.engine.smoke_get_grad(0)
    c = lay['smoke']['cells']
    assert gq.sum() == len(c) and (gq[c[:, 0], c[:, 1], c[:, 2], 0] == 1).all() and not gv.any()
    for k in (0, 7, 8):
        g[:] = 0; g[k] = 1.0
        with pytest.raises(_capi.FeEngineError):
            env.obs_backward(g, f=0)
    env.taichi_env.reset_grad()


@pytest.mark.parametrize('name', sorted(REGISTRY))
def test_action_bounds_and_the_policy_output(name, oracle32, oracle64, circulation):
    env = circulation if name == 'Circulation-v0' else _small_env(name, oracle32)
    if env.taichi_env.agent is None:                             # (WaterBlock: nothing to command, no policy to build)
        assert env.action_space is None
        return
    ad = env.taichi_env.agent.action_dim
    lo, hi = env.action_bounds()
    assert lo.shape == hi.shape == (ad,)
    pol = ObsPolicy(env, hidden=8, seed=3, use_agent_state=name != 'Circulation-v0')
    rng = np.random.RandomState(11)
    o0 = np.asarray(env._get_obs(), np.float64)
    t = lambda a: torch.as_tensor(a, dtype=pol.dtype)
    if name != 'Circulation-v0':
        r0, r1 = float(env.action_range[0]), float(env.action_range[1])
        assert (lo == r0).all() and (hi == r1).all()
        mid, half = t(0.5 * (r0 + r1)), t(0.5 * (r1 - r0))       # the scalar form ObsPolicy had
        for _ in range(3):
            o = t(o0 + rng.normal(size=o0.shape) * 0.01)
            want = mid + half * torch.tanh(pol.net((o - pol.shift) * pol.gain))
            assert torch.equal(pol(o), want)
        return
    assert (lo[FIXED] == DEMO_ROW[FIXED]).all() and (hi[FIXED] == DEMO_ROW[FIXED]).all()
    assert (lo[4], hi[4]) == (-0.1, 0.1) and lo[7] > 0
    seen = []
    for _ in range(5):
        o = t(o0 + rng.normal(size=o0.shape) * 10.0).requires_grad_(True)
        a = pol(o)
        assert (a.detach().numpy()[FIXED] == t(DEMO_ROW).numpy()[FIXED]).all()
        assert abs(float(a[4].detach())) <= 0.1
        seen.append(float(a[4].detach()))
        a[FIXED].sum().backward()
        assert not o.grad.any()                                  # the fixed entries carry no gradient
    assert len(set(seen)) > 1                                    # entry 4 is the policy's to command


def test_a_nonpositive_radius_bound_on_an_aircon_is_refused(circulation):
    lo, hi = circulation.action_bounds()
    for bad in (0.0, -0.1):
        lo7 = lo.copy(); lo7[7] = bad
        with pytest.raises(AssertionError, match='radius'):
            ObsPolicy(circulation, hidden=8, action_lo=lo7, action_hi=hi)
    ObsPolicy(circulation, hidden=8, action_lo=lo, action_hi=hi)
    lo7 = lo.copy(); lo7[7] = 0.01
    ObsPolicy(circulation, hidden=8, action_lo=lo7, action_hi=hi)   # explicit bounds with a positive radius pass
