"""Closed-loop policies trained through the simulator: a_i = pi_theta(o_i), back-propagation through time.

The open-loop Solver differentiates a rollout with respect to a table of actions.  Here the action of step i is a function of the
observation of the frame the step starts from, so the reverse sweep has one more edge per step: after step i has been differentiated
back to its first frame f_i, dL/da_i (the engine's gabuf[i]) goes through the policy -- torch.autograd accumulates theta.grad and yields
dL/do_i -- and dL/do_i is added to the adjoint of frame f_i (FluidEnv.obs_backward) before the sweep goes on to step i - 1.

With enable_device_obs() on the HIP engine nothing of that crosses PCIe: the observation is gathered on the GPU, the action is read from
the policy's output tensor, gabuf[i] is copied to a device tensor and the cotangent rows are scattered by the engine
(include/fluidengine_ext.h: fe_obs_add_grad_dev and friends).  Without it the same loop runs on host arrays and dense add_grad, on every
engine, the CPU oracles included.  The reference has no counterpart."""
from time import time

import numpy as np
import torch

from fluidlab_amd._capi import FE_EFF_AIRCON


def _engine_torch(env):
    """(dtype, device) of the tensors that match the env's engine: fp32 on its GPU for the HIP engine, the oracle's precision on the CPU"""
    eng = env.taichi_env.simulator.engine
    if eng.elib.backend.startswith('hip'):
        return torch.float32, torch.device('cuda', eng.device)
    return (torch.float64 if eng.dtype == np.float64 else torch.float32), torch.device('cpu')


class ObsPolicy(torch.nn.Module):
    """An MLP from the observation vector to the action: tanh(.) scaled entry by entry into env.action_bounds() (action_lo= / action_hi=
    override them), so no clipping is needed downstream; an entry with lo == hi comes out as exactly that value and carries no gradient.
    The lower bound of an AirCon's radius (its entry 7) must be positive.  A layout with a 'smoke' entry (CirculationEnv) is taken as it
    is: scale 1 on the field's rows.  A layout with 'fields' (FluidEnv.enable_field_obs) gets one more constant per field block: the block's
    largest density value in o_0, or 1 if that is 0 -- fixed, not trained.
    The input is (o - o_0) / scale with o_0 the observation the policy was built on and scale the spread of o_0's positions on the position
    entries, 1 elsewhere -- fixed, not trained.  use_agent_state=False masks the tool's pose (and whatever else its state holds) out of the
    input, `used` flags are always masked: they carry no gradient.  input_gain multiplies the normalised input (how strongly the first
    layer sees a change of the scene: within a few steps particles move by thousandths of the scene's size).  actions_p, if given, is the tool's start pose, applied (not trained)
    at the start of every rollout like the open-loop policies' pose row."""

    def __init__(self, env, hidden=64, n_layers=2, use_agent_state=True, actions_p=None, input_gain=1.0, seed=0, action_lo=None, action_hi=None):
        super().__init__()
        self.dtype, self.device = _engine_torch(env)
        layout = env.obs_layout()
        o0 = np.asarray(env._get_obs(), np.float64)
        assert o0.shape == (layout['size'],), (o0.shape, layout['size'])
        mask, scale = np.ones_like(o0), np.ones_like(o0)
        xs = np.concatenate([o0[b['x']] for b in layout['bodies']]) if layout['bodies'] else np.zeros((0,))
        spread = float(xs.reshape(-1, 3).std(axis=0).max()) if xs.size else 1.0
        for b in layout['bodies']:
            scale[b['x']] = spread if spread > 0 else 1.0
            mask[b['used']] = 0.0
        for s_pose, s_extra in zip(layout['agent'], layout['extra']):
            if not use_agent_state:
                mask[s_pose] = 0.0
            if s_extra is not None:
                mask[s_extra] = 0.0 if not use_agent_state else mask[s_extra]
        for fs in layout.get('fields', []):                      # a field block: one constant, the block's largest density value in o_0
            dmax = float(o0[fs['slice']].reshape(fs['shape'])[0].max())
            scale[fs['slice']] = dmax if dmax > 0 else 1.0
        self.use_agent_state = bool(use_agent_state)
        self.actions_p = None if actions_p is None else np.asarray(actions_p, np.float64)
        t = lambda a: torch.as_tensor(a, dtype=self.dtype, device=self.device)
        self.register_buffer('shift', t(o0))
        self.register_buffer('gain', t(float(input_gain) * mask / scale))
        action_dim = env.taichi_env.agent.action_dim
        lo, hi = env.action_bounds()
        lo = np.array(lo if action_lo is None else action_lo, np.float64).reshape(-1)
        hi = np.array(hi if action_hi is None else action_hi, np.float64).reshape(-1)
        assert lo.shape == hi.shape == (action_dim,) and (lo <= hi).all(), (lo, hi, action_dim)
        at = 0
        for e in env.taichi_env.agent.effectors:                 # the jet's impulse is exp(-dist / r): r <= 0 must not be commandable
            if e.abi_type == FE_EFF_AIRCON and e.action_dim > 7:
                assert lo[at + 7] > 0, f'ObsPolicy: the lower bound of an AirCon\'s radius (action entry {at + 7}) must be > 0, got {lo[at + 7]}'
            at += e.action_dim
        self.register_buffer('act_mid', t(0.5 * (lo + hi)))
        self.register_buffer('act_half', t(0.5 * (hi - lo)))
        gen = torch.Generator().manual_seed(int(seed))
        dims = [layout['size']] + [int(hidden)] * int(n_layers) + [action_dim]
        layers = []
        for k in range(len(dims) - 1):
            lin = torch.nn.Linear(dims[k], dims[k + 1])
            with torch.no_grad():                                # (seeded on the CPU in fp64, whatever the module's device and dtype)
                bound = 1.0 / np.sqrt(dims[k])
                lin.weight.copy_((torch.rand(lin.weight.shape, generator=gen, dtype=torch.float64) * 2 - 1) * bound)
                lin.bias.copy_((torch.rand(lin.bias.shape, generator=gen, dtype=torch.float64) * 2 - 1) * bound)
            layers.append(lin)
            if k < len(dims) - 2:
                layers.append(torch.nn.Tanh())
        self.net = torch.nn.Sequential(*layers).to(dtype=self.dtype, device=self.device)

    def forward(self, obs):
        return self.act_mid + self.act_half * torch.tanh(self.net((obs - self.shift) * self.gain))


class ClosedLoopSolver:
    """forward_backward(sim_state): one rollout under the policy with loss, then the reverse sweep with the policy in it; the gradient is
    left in the parameters' .grad.  solve(): cfg.n_iters steps of torch.optim.Adam (cfg.optim.lr and betas as the open-loop configs).
    check_finite=True: the summary of the frame the rollout starts from and, after every forward step, of the new frame is read
    (smoke_summary for an environment with a smoke field, frame_summary otherwise) and a non-finite value raises FloatingPointError
    instead of travelling on through the rollout.  That is one wait for the engine's stream per step -- the device road otherwise enqueues a step without waiting -- so it is off by default."""

    def __init__(self, env, policy, cfg=None, logger=None, check_finite=False):
        self.env, self.policy, self.cfg, self.logger = env, policy, cfg, logger
        self.check_finite = bool(check_finite)
        self.skip_obs_backward = False                           # (tests: the direct term sum_i J_pi^T dL/da_i alone)

    # ---- the three crossings of a step
    def _device_road(self):
        env = self.env
        eng = env.taichi_env.simulator.engine
        return bool(env._device_obs) and eng.elib.backend.startswith('hip') and eng.elib.has_ext

    def _observe(self):
        """the observation of the current frame as a leaf tensor of the policy's dtype on its device"""
        env, pol = self.env, self.policy
        te = env.taichi_env
        agent = te.agent
        if self._device_road() and hasattr(env, 'observe_dev'):  # (CirculationEnv: the whole vector from one launch)
            obs = env.observe_dev()
        elif self._device_road() and all(e.state_dim == 7 for e in agent.effectors) and te.particles is not None:
            sim = te.simulator
            eng, f, n = sim.engine, sim.cur_substep_local, sim.engine.n_obs
            layout = env.obs_layout()
            parts = []
            if layout['bodies']:
                x = torch.empty((n, 3), dtype=torch.float32, device=pol.device); v = torch.empty_like(x)
                used = torch.empty((n,), dtype=torch.int32, device=pol.device)
                eng.get_obs_dev(f, x, v, used)
                for b in layout['bodies']:
                    lo, hi = b['rows']
                    parts += [x[lo:hi].reshape(-1), v[lo:hi].reshape(-1), used[lo:hi].to(torch.float32)]
            for e in agent.effectors:
                s7 = torch.empty((7,), dtype=torch.float32, device=pol.device)
                eng.eff_get_state_dev(e.index, f, s7)
                parts.append(s7)
            for k in range(len(layout.get('fields', []))):       # the fields are rasterised where the frame is: no frame is downloaded
                parts.append(eng.field_obs_dev(f, k).reshape(-1))
            obs = torch.cat(parts)
        else:
            obs = torch.as_tensor(np.asarray(env._get_obs()), dtype=pol.dtype, device=pol.device)
        return obs.requires_grad_(torch.is_grad_enabled())

    def _action_for_engine(self, a):
        return a.detach() if self._device_road() else a.detach().cpu().numpy()

    def _action_grad(self, i):
        """dL/da_i: row i of every effector's gabuf, concatenated like the action"""
        agent, pol = self.env.taichi_env.agent, self.policy
        rows = []
        for e in agent.effectors:
            if e.action_dim == 0:
                continue
            if self._device_road():
                out = torch.empty((1, e.action_dim), dtype=torch.float32, device=pol.device)
                e.engine.eff_get_action_grad_dev(e.index, i, 1, out)
                rows.append(out[0])
            else:
                rows.append(torch.as_tensor(e.get_action_grad(i, 1)[0], dtype=pol.dtype, device=pol.device))
        return torch.cat(rows)

    # ---- one pass
    def _forward(self, sim_state, grad_enabled):
        env, pol = self.env, self.policy
        te = env.taichi_env
        sim = te.simulator
        te.set_state(sim_state, grad_enabled=grad_enabled)
        if pol.actions_p is not None:
            te.apply_agent_action_p(pol.actions_p)
        cur_horizon = te.loss.temporal_range[1]
        n_act = min(cur_horizon, env.horizon_action)
        obs, act, frame = [], [], []

        def finite(where):
            rec = te.smoke_summary() if te.smoke_field is not None else te.frame_summary()
            if rec['n_nonfinite'] > 0:
                raise FloatingPointError(f"closed-loop rollout: {rec['n_nonfinite']} non-finite cells or particles in the frame {where}")
        if self.check_finite:                                    # (the smoke solver samples the grid's edge for a non-finite back-trace: a step can
            finite('the rollout starts from')                    #  swallow what it was given, so the frame it starts from is looked at as well)
        for i in range(cur_horizon):
            if i < n_act:
                frame.append(sim.cur_substep_local)
                o = self._observe()
                a = pol(o)
                obs.append(o); act.append(a)
                te.step(self._action_for_engine(a), exact=True)
            else:
                te.step(None)
            if self.check_finite:
                finite(f'after step {i}')
        return obs, act, frame

    def rollout(self, sim_state):
        """the forward pass alone, without keeping anything for a reverse sweep: the loss of the policy as it stands"""
        with torch.no_grad():
            self._forward(sim_state, grad_enabled=False)
        return self.env.taichi_env.get_final_loss()

    def forward_backward(self, sim_state):
        env, pol = self.env, self.policy
        te = env.taichi_env
        t1 = time()
        obs, act, frame = self._forward(sim_state, grad_enabled=True)
        cur_horizon, n_act = te.loss.temporal_range[1], len(act)
        loss_info = te.get_final_loss()
        t2 = time()
        te.reset_grad()
        te.get_final_loss_grad()
        for p in pol.parameters():
            p.grad = None
        for i in range(cur_horizon - 1, -1, -1):
            if i >= n_act:
                te.step_grad(None)
                continue
            te.step_grad(self._action_for_engine(act[i]), exact=True)
            # the kept o_i and a_i: a replayed chunk would not give the same bits back
            torch.autograd.backward(act[i], self._action_grad(i))
            if not self.skip_obs_backward:
                env.obs_backward(obs[i].grad, f=frame[i])        # before the next step_grad: its memory_from_cache carries frame 0's adjoint over
        t3 = time()
        loss_info['forward_s'], loss_info['backward_s'] = t2 - t1, t3 - t2
        return loss_info

    def grad_vector(self):
        """the parameters' gradients as one fp64 vector (parameter order)"""
        return np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().double().reshape(-1).numpy()
                               for p in self.policy.parameters()])

    def solve(self, callback=None):
        cfg = self.cfg
        te = self.env.taichi_env
        init_state = te.get_state()
        oc = cfg.optim
        opt = torch.optim.Adam(self.policy.parameters(), lr=float(oc.lr), betas=(float(oc.get('beta_1', 0.9)), float(oc.get('beta_2', 0.999))))
        for iteration in range(cfg.n_iters):
            if self.logger is not None:
                self.logger.save_policy(self.policy.state_dict(), iteration)
            loss_info = self.forward_backward(init_state['state'])
            print(f"=======> forward: {loss_info['forward_s']:.2f}s backward: {loss_info['backward_s']:.2f}s")
            opt.step()
            loss_info['iteration'] = iteration
            if self.logger is not None:
                loss_info['lr'] = float(oc.lr)
                self.logger.log(iteration, loss_info)
            if callback is not None:
                callback(iteration, loss_info, self.policy)
        return self.policy


def solve_closed_loop(env, logger, cfg, check_finite=False, **policy_kwargs):
    env.reset()
    p0 = cfg.init_range.p[0] if 'init_range' in cfg else None
    policy = ObsPolicy(env, actions_p=p0, **policy_kwargs)
    return ClosedLoopSolver(env, policy, cfg, logger, check_finite=check_finite).solve()
