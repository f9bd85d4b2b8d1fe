"""Cost of one closed-loop step, forward and backward, on the device road and on the dense road (optimizer/closed_loop.py,
FluidEnv.obs_backward), at the shipped sizes of GatheringEasy-v0 and Transporting-v0, and of the observation adjoint alone --
fe_obs_add_grad_dev with the ~200-row list against fe_add_grad_dev with two dense [N, 3] arrays on the benchmark block (WaterBlock-v0);
for the smoke field, fe_smoke_cells_add_grad_dev with the rows of Circulation-v0's observation lattice (128^3 smoke grid, 1,352 cells)
against fe_smoke_add_grad with two dense host fields.  With --only Circulation also: fe_smoke_obs_get_dev against _get_obs() with
enable_device_obs(), fe_smoke_obs_add_grad_dev against the three calls it replaces, and one closed-loop step of the shipped Circulation-v0
(128^3, 1,352-cell lattice) on the device road and on the dense road, the smoke summary checked for non-finite cells after every step.
  forward = observation of the current frame, the policy, TaichiEnv.step(action)
  backward = TaichiEnv.step_grad(action), dL/da from the engine, torch.autograd.backward through the policy, FluidEnv.obs_backward
Wall clock per call with the engine's stream (and torch's) drained before the clock starts and again before it stops; 5 warm-up calls,
then the median of 30.
usage: python scripts/closed_loop_cost.py [--commit TEXT] [--out FILE] [--lib PATH] [--small] [--only NAME]
  --only NAME one environment alone (a substring of its name; WaterBlock-v0 and Circulation-v0 are the two scatter measurements)
  --lib PATH  another library with the engine ABI (an oracle build has no device road: only the dense road is measured)
  --small     reduced scenes (a dry run of the script)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd import _capi  # noqa: E402
from fluidlab_amd.envs import make  # noqa: E402
from fluidlab_amd.optimizer.closed_loop import ClosedLoopSolver, ObsPolicy  # noqa: E402


def timed(sync, fn, warm=5, n=30):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        sync()
        t0 = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t0)
    return 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts)


def fmt(t):
    return f'{t[0]:10.1f} ({t[1]:.1f} .. {t[2]:.1f})'


CIRCULATION_SMALL = dict(res=32, solver_iters=10, horizon=12, detectors=[[6, 16, 21], [9, 16, 21], [6, 16, 10], [26, 16, 16], [24, 16, 20], [20, 16, 8]])
CIRCULATION_P = [0.55, 0.5, 0.35, 0.0, 0.0, 0.0, 0.0, 0.0]       # the start pose of configs/exp_circulation.yaml


def closed_loop_step(name, lib, device_obs, small, emit, make_kw=None, start_pose=None, check_finite=False):
    """make_kw: the environment's keywords instead of the particle scenes' (Circulation-v0); start_pose: applied before the first step;
    check_finite: the smoke summary is read after every forward step, outside the clock, and a non-finite cell ends the measurement"""
    import torch
    kw = dict(quality=0.5, particle_density=3e4, horizon=12) if small else {}
    if small and name.startswith('Transporting'):
        kw.update(n_pool=400, particle_density=2e5)
    if make_kw is not None:
        kw = dict(make_kw)
    env = make(name, seed=0, loss=True, engine_lib=lib, ckpt_dest='cpu', **kw)
    if device_obs:
        env.enable_device_obs()
    te = env.taichi_env
    sim = te.simulator
    pol = ObsPolicy(env, hidden=64, use_agent_state=lib.has_ext, seed=1)          # (an oracle library has no entry for the pose adjoint)
    sol = ClosedLoopSolver(env, pol)
    assert sol._device_road() == device_obs
    te.set_state(te.get_state()['state'], grad_enabled=True)
    if start_pose is not None:
        te.apply_agent_action_p(np.asarray(start_pose, np.float64))
    kept = {}

    def finite():
        if check_finite:
            rec = te.smoke_summary()
            if rec['n_nonfinite'] > 0:
                raise FloatingPointError(f"{name}: {rec['n_nonfinite']} non-finite cells after a closed-loop step")

    def sync():
        sim.engine.sync()
        if pol.device.type == 'cuda':
            torch.cuda.synchronize(pol.device)

    def forward():
        kept['f'] = sim.cur_substep_local
        kept['o'] = sol._observe()
        kept['a'] = pol(kept['o'])
        te.step(sol._action_for_engine(kept['a']), exact=True)

    def backward():
        i = sim.cur_step_global - 1
        te.step_grad(sol._action_for_engine(kept['a']), exact=True)
        torch.autograd.backward(kept['a'], sol._action_grad(i))
        env.obs_backward(kept['o'].grad, f=kept['f'])

    forward()                                                    # one step with its loss, so that the reverse sweep has something to start from
    finite()
    te.loss.temporal_range = [0, 1]
    te.get_final_loss(); te.reset_grad(); te.get_final_loss_grad()
    backward()
    fw, bw = [], []
    for k in range(35):
        sync(); t0 = time.perf_counter(); forward(); sync(); t1 = time.perf_counter()
        finite()
        sync(); t1b = time.perf_counter(); backward(); sync(); t2 = time.perf_counter()
        t2 -= t1b - t1
        if k >= 5:
            fw.append(t1 - t0); bw.append(t2 - t1)
    us = lambda ts: (1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts))
    emit(f'  {name:18s} N {sim.n_particles:7d} obs {env.obs_layout()["size"]:5d}  {"device road" if device_obs else "dense road ":11s}  forward {fmt(us(fw))}   backward {fmt(us(bw))}')
    sim.engine.close()


def scatter_alone(lib, small, emit):
    import torch
    kw = dict(quality=0.5, n_particles=4096) if small else {}
    env = make('WaterBlock-v0', horizon=2, engine_lib=lib, **kw)
    env.enable_device_obs()
    sim = env.taichi_env.simulator
    eng = sim.engine
    env.taichi_env.step(None)
    f, N, n = sim.cur_substep_local, sim.n_particles, eng.n_obs
    dev = torch.device('cuda', eng.device)
    rng = np.random.RandomState(1)
    gx, gv = (torch.as_tensor(rng.normal(size=(n, 3)).astype(np.float32), device=dev) for _ in range(2))
    ids = torch.as_tensor(np.concatenate(env._obs_ids()[0]).astype(np.int64), device=dev)
    GX, GV = (torch.zeros((N, 3), dtype=torch.float32, device=dev) for _ in range(2))
    GX[ids] = gx; GV[ids] = gv

    def sync():
        eng.sync(); torch.cuda.synchronize(dev)
    eng.reset_grad()
    a = timed(sync, lambda: eng.obs_add_grad_dev(f, gx, gv))
    b = timed(sync, lambda: eng.add_grad_dev(f, gx=GX, gv=GV))
    emit(f'WaterBlock-v0 (n_grid {sim.n_grid}, N {N}), frame {f}, list of {n} rows:')
    emit(f'  fe_obs_add_grad_dev ({n} rows)              {fmt(a)}')
    emit(f'  fe_add_grad_dev (two dense [N, 3] arrays)   {fmt(b)}')
    eng.close()


def smoke_scatter_alone(lib, small, emit):
    import torch
    env = make('Circulation-v0', seed=0, loss=True, engine_lib=lib, ckpt_dest='cpu', **(CIRCULATION_SMALL if small else {}))
    env.enable_device_obs()                                      # registers the observation lattice as cell list OBS_LIST
    te = env.taichi_env
    sim, sf = te.simulator, te.smoke_field
    eng = sim.engine
    te.set_state(te.get_state()['state'], grad_enabled=True)
    te.apply_agent_action_p(np.asarray(CIRCULATION_P, np.float64))
    te.step(np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.02, 0.04]))
    s, qd, ng = sim.cur_step_local, sf.q_dim, sf.n_grid
    cells = np.stack(np.meshgrid(np.arange(0, ng, 10), np.arange(sf.lower_y, sf.higher_y), np.arange(0, ng, 10), indexing='ij'), axis=-1).reshape(-1, 3)
    n = len(cells)
    dev = torch.device('cuda', eng.device)
    rng = np.random.RandomState(1)
    rv, rq = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, qd)).astype(np.float32)
    gv, gq = torch.as_tensor(rv, device=dev), torch.as_tensor(rq, device=dev)

    def dense():
        GV, GQ = np.zeros((ng, ng, ng, 3), np.float32), np.zeros((ng, ng, ng, qd), np.float32)
        np.add.at(GV, (cells[:, 0], cells[:, 1], cells[:, 2]), rv)
        np.add.at(GQ, (cells[:, 0], cells[:, 1], cells[:, 2]), rq)
        return GV, GQ
    GV, GQ = dense()

    def sync():
        eng.sync(); torch.cuda.synchronize(dev)
    eng.smoke_reset_grad()
    a = timed(sync, lambda: eng.smoke_cells_add_grad(env.OBS_LIST, s, gv=gv, gq=gq))
    b = timed(sync, lambda: eng.smoke_add_grad(s, gv=GV, gq=GQ))
    c = timed(sync, lambda: eng.smoke_add_grad(s, *dense()))
    emit(f'Circulation-v0 (smoke grid {ng}^3, q_dim {qd}), smoke frame {s}, list of {n} cells ({4 * n * (3 + qd)} B of rows, {GV.nbytes + GQ.nbytes} B of dense fields):')
    emit(f'  fe_smoke_cells_add_grad_dev ({n} rows)                   {fmt(a)}')
    emit(f'  fe_smoke_add_grad (two dense host fields, built once)     {fmt(b)}')
    emit(f'  the same with the fields built per call (np.add.at)       {fmt(c)}')
    # the whole observation vector and its cotangent, one launch each, against the calls they replace
    e, f = env.agent.effectors[0], sim.cur_substep_local
    m = eng.smoke_obs_size(env.OBS_LIST)
    g = torch.as_tensor(rng.normal(size=m).astype(np.float32), device=dev)
    g7 = g[:7].contiguous()
    gs, gr = float(g[7]), float(g[8])
    out = torch.empty((m,), dtype=torch.float32, device=dev)

    def composed():
        eng.smoke_cells_add_grad(env.OBS_LIST, s, gv=gv, gq=gq)
        eng.eff_add_state_grad_dev(e.index, f, g7)
        eng.eff_add_sr_grad(e.index, f, gs, gr)
    o1 = timed(sync, lambda: eng.smoke_obs_get(env.OBS_LIST, s, e.index, f, out=out))
    o2 = timed(sync, env._get_obs)
    a1 = timed(sync, lambda: eng.smoke_obs_add_grad(env.OBS_LIST, s, e.index, f, g))
    a2 = timed(sync, composed)
    emit(f'  fe_smoke_obs_get_dev ({m} words, one launch)               {fmt(o1)}')
    emit(f'  _get_obs() with enable_device_obs() (state, s, r, gather)   {fmt(o2)}')
    emit(f'  fe_smoke_obs_add_grad_dev (one launch)                      {fmt(a1)}')
    emit(f'  cells_add_grad_dev + eff_add_state_grad_dev + add_sr_grad   {fmt(a2)}')
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--lib', default=None)
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    lines = []

    def emit(text):
        lines.append(text)
        print(text, flush=True)
    lib = _capi.EngineLib(args.lib) if args.lib else _capi.load_hip()
    emit(f'commit {args.commit}')
    emit(f'backend {lib.backend}; microseconds per call, wall clock, streams drained before and after: median (min .. max) of 30 after 5 warm-up calls')
    emit(f'one closed-loop step (ObsPolicy hidden 64, use_agent_state={lib.has_ext}):')
    for name in (n for n in ('GatheringEasy-v0', 'Transporting-v0') if args.only in n):
        for device_obs in ((True, False) if lib.has_ext else (False,)):
            closed_loop_step(name, lib, device_obs, args.small, emit)
    if lib.has_ext and args.only in 'WaterBlock-v0':
        scatter_alone(lib, args.small, emit)
    if lib.has_ext and args.only in 'Circulation-v0':
        smoke_scatter_alone(lib, args.small, emit)
    if args.only and args.only in 'Circulation-v0':              # (the full-size closed loop: asked for by name, with the finiteness check on)
        for device_obs in ((True, False) if lib.has_ext else (False,)):
            closed_loop_step('Circulation-v0', lib, device_obs, args.small, emit, make_kw=CIRCULATION_SMALL if args.small else {},
                             start_pose=CIRCULATION_P, check_finite=lib.has_ext)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
