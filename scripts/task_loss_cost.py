"""Cost of one task-loss step at the shipped sizes of Transporting-v0 ('diff'), Mixing-v0 and GatheringEasy-v0 (64^3 grid, particle_density 1e6),
through the Python stack: the torch path of HostLoss (frame download into torch, a chain of small launches, a host synchronisation per
partial value; the pair terms through host_loss.pairwise_l1) against the loss-term program in the engine (HostLoss.enable_device_loss:
fe_task_loss_step / fe_task_loss_step_grad, include/fluidengine_ext.h).  The environment is rolled out 20 steps, then the loss of the
current step is evaluated (forward) and differentiated (backward) on the current frame.
Wall clock per call with the engine's stream drained before the clock starts and again before it stops; 5 warm-up calls, then the median of 30.
usage: python scripts/task_loss_cost.py [--commit TEXT] [--out FILE] [--steps N]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd.envs import make  # noqa: E402
from fluidlab_amd.utils.config import load_config  # noqa: E402


def transporting(pol):
    pol.actions_p[:] = [0.42, 0.5, 0.5, 0.0, 0.0, 0.0]
    pol.actions_v[:, 5] = 0.0005


def mixing(pol):
    pol.actions_p[:] = [0.5, 0.62, 0.5]
    pol.actions_v[:, 0] = 0.003


def gathering(pol):
    pol.actions_v[:, 0] = 0.003


ENVS = (('Transporting-v0', 'configs/exp_transporting.yaml', transporting), ('Mixing-v0', 'configs/exp_mixing.yaml', mixing),
        ('GatheringEasy-v0', 'configs/exp_gathering_easy.yaml', gathering))


def timed(eng, fn, warm=5, n=30):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        eng.sync()
        t0 = time.perf_counter(); fn(); eng.sync(); ts.append(time.perf_counter() - t0)
    return 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts)


def sets(loss, used):
    """what the loss runs over, in words"""
    name = type(loss).__name__
    if name == 'TransportingLoss':
        return f'{int(used[:loss.n_particles_water].sum())} used of {loss.n_particles_water} water x {loss.obj_end - loss.obj_start} cube particles'
    if name == 'MixingLoss':
        return f'all ordered pairs of {loss.n_particles_milk} milk particles'
    return f'{int((used & (np.asarray(loss.sim.particles_i.mat.to_numpy()) == loss.matching_mat)).sum())} particles of the matching material'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--steps', type=int, default=20)
    args = ap.parse_args()
    lines = []

    def emit(text):
        lines.append(text)
        print(text, flush=True)
    emit(f'commit {args.commit}')
    emit('microseconds per call, wall clock, stream drained before and after: median (min .. max) of 30 after 5 warm-up calls')
    emit(f'{"":34s} {"torch path (parent)":>34s}   {"device path (loss-term program)":>34s}')
    for name, cfg_file, prepare in ENVS:
        env = make(name, seed=0, loss=True, horizon=args.steps + 2, max_substeps_local=None)
        te = env.taichi_env
        loss, sim = te.loss, te.simulator
        eng = sim.engine
        loss.temporal_range[1] = env.horizon
        cfg = load_config(cfg_file).SOLVER
        pol = env.trainable_policy(cfg.optim, cfg.init_range)
        prepare(pol)
        env.enable_device_loss()
        te.set_state(te.get_state()['state'], grad_enabled=True)
        te.apply_agent_action_p(pol.get_actions_p())
        for i in range(args.steps):
            te.step(pol.get_action_v(i, agent=te.agent, update=True))
        s, f = sim.cur_step_global - 1, sim.cur_substep_local
        used = np.zeros((sim.n_particles,), np.int32)
        eng.get_frame(f, used=used)
        emit(f'{name}: backend {eng.elib.backend}, n_grid {sim.n_grid}, N {sim.n_particles}, frame {f}; {sets(loss, used > 0)}; '
             f'task_pair_chunk {int(eng.get_option("task_pair_chunk"))} (0 = chosen by the engine)')
        eng.reset_grad()
        res = {}
        for path, on in (('torch', False), ('device', True)):
            loss._device_loss = on
            res[path] = (timed(eng, lambda: loss.compute_step_loss(s, f)), timed(eng, lambda: loss.compute_step_loss_grad(s, f)))
        loss._device_loss = True
        for k, what in enumerate(('forward  loss step', 'backward loss step')):
            a, b = res['torch'][k], res['device'][k]
            emit(f'  {what:32s} {a[0]:12.1f}   ({a[1]:.1f} .. {a[2]:.1f})   {b[0]:12.1f}   ({b[1]:.1f} .. {b[2]:.1f})   torch / device {a[0] / b[0]:.2f}')
        del env, te, loss, sim, eng
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
