"""The translation of the five task losses into loss-term programs (HostLoss.device_terms + extra_step_value), checked without a GPU: on the
fp64 oracle, after a few steps of each reduced environment, the fp64 numpy interpreter of the program (term_program.eval_terms_numpy, pairs by
brute force) plus the extra hook is compared with the class's own step_value on the same frame.

Value: within 1e-12 x sum |terms| (both are fp64 sums of a few thousand equal terms in different orders: (n - 1) 2^-53 ~ 5e-13 for n = 5,000).
Gradient: equal where it is a sign or a count times a weight (the same fp64 products in the same order), within 1e-15 relative for the
squared distance of GatheringO (2 d w: the same two products; the bound allows one rounding of difference all the same)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from fluidlab_amd.fluidengine.losses.term_program import eval_terms_numpy  # noqa: E402
from fluidlab_amd.utils.config import load_config  # noqa: E402


def _prep_none(pol):
    pass


def _prep_gathering(pol):
    pol.actions_v[:, 0] = 0.003


def _prep_pouring(pol):
    pol.actions_v[:, 5] = 0.02


def _prep_transporting(pol):
    pol.actions_p[:] = [0.42, 0.5, 0.5, 0.0, 0.0, 0.0]
    pol.actions_v[:, 5] = 0.002


def _prep_mixing(pol):
    pol.actions_p[:] = [0.5, 0.62, 0.5]
    pol.actions_v[:, 0] = 0.005


CASES = {
    'gathering_easy': ('GatheringEasy-v0', 'configs/exp_gathering_easy.yaml', _prep_gathering, {}),
    'gathering_o': ('GatheringO-v0', 'configs/exp_gatheringO.yaml', _prep_gathering, {}),
    'pouring': ('Pouring-v0', 'configs/exp_pouring.yaml', _prep_pouring, dict(horizon=10)),
    'pouring_default': ('Pouring-v0', 'configs/exp_pouring.yaml', _prep_pouring, dict(horizon=10, loss_type='default')),
    'transporting': ('Transporting-v0', 'configs/exp_transporting.yaml', _prep_transporting, dict(horizon=10, n_pool=400, particle_density=2e5)),
    'mixing': ('Mixing-v0', 'configs/exp_mixing.yaml', _prep_mixing, dict(horizon=10)),
}


def build_env(case, engine_lib):
    """the reduced environment of tests/test_host_env.py and a policy with that file's actions"""
    import test_host_env as H
    name, cfg_file, prepare, kw = CASES[case]
    env = H._gathering(engine_lib) if case == 'gathering_easy' else H._small(name, engine_lib, **kw)
    cfg = load_config(cfg_file).SOLVER
    pol = env.trainable_policy(cfg.optim, cfg.init_range)
    prepare(pol)
    if hasattr(env.taichi_env.loss, 'temporal_range'):
        env.taichi_env.loss.temporal_range[1] = env.horizon
    return env, pol, cfg


def roll(env, pol, n_steps):
    te = env.taichi_env
    te.set_state(te.get_state()['state'], grad_enabled=True)
    te.apply_agent_action_p(pol.get_actions_p())
    for i in range(n_steps):
        te.step(pol.get_action_v(i, agent=te.agent, update=True) if i < env.horizon_action else None)


@pytest.mark.parametrize('case', list(CASES))
def test_program_reproduces_step_value(oracle64, case):
    env, pol, _ = build_env(case, oracle64)
    te = env.taichi_env
    loss, sim = te.loss, te.simulator
    roll(env, pol, 3)
    f = sim.cur_substep_local
    x, used = loss.frame(f)
    mat = np.asarray(loss.particle_mat)
    terms = loss.device_terms()
    assert terms is not None and 1 <= len(terms) <= 8
    ref = getattr(loss, 'init_particle_pos', None)
    steps = [sim.cur_step_global - 1]
    if case.startswith('pouring'):
        steps.append(loss.max_loss_steps - 1)                  # the step with the 'diff' attraction beside the program
        assert ref is not None
    for s in steps:
        v_host, g_host = loss.step_value(s, f, x, used, True)
        vals, g = eval_terms_numpy(terms, x, used, mat, ref, True)
        ev, eg = loss.extra_step_value(s, f, True)
        if eg is not None:
            g = g + eg
        total, scale = float(vals.sum()) + ev, float(np.abs(vals).sum()) + abs(ev)
        print(f'{case} step {s}: host {v_host!r} program {total!r} (terms {vals!r}, extra {ev!r}) err {abs(total - v_host)!r} bound {1e-12 * scale!r}')
        assert scale > 0 and np.abs(g_host).max() > 0
        assert abs(total - v_host) <= 1e-12 * scale
        if case == 'gathering_o':
            assert np.all(np.abs(g - g_host) <= 1e-15 * np.abs(g_host))
        else:
            assert np.array_equal(g, g_host)
    if case == 'pouring':
        assert eg is not None and np.abs(eg).max() > 0         # the attraction really ran on the last step
    if case == 'transporting':
        assert int(used[:loss.n_particles_water].sum()) > 0 and len(terms) == 2 and vals[1] > 0
