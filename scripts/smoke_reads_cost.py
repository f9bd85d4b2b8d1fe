"""Cost of the smoke-field reads that stay on the GPU (include/fluidengine_ext.h: fe_smoke_cells_*, fe_smoke_loss_*, fe_smoke_summary) in
Circulation-v0 at its shipped size: 128^3 smoke grid, q_dim 1, fifteen detectors, after two steps.  Three pairs, the existing road against
the device road of the same build:
  CirculationEnv._get_obs()                 get_state_RL (v, v_tmp, div, p, q whole)        against   the lattice cell list (fe_smoke_cells_get)
  CirculationLoss.step() / step_grad()      q_at / add_q_grad_at (q down, a dense field up)  against   fe_smoke_loss_step / _step_grad
  TaichiEnv.smoke_summary()                 fe_smoke_summary                                 against   fe_smoke_get_frame of v and q, reduced in numpy
Wall clock per call with the engine's stream drained before and after; 3 warm-up calls, then the median of 30.
usage: python scripts/smoke_reads_cost.py [--commit TEXT] [--out FILE] [--res N]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd.envs import make  # noqa: E402


def timed(eng, fn, warm=3, n=30):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        eng.sync()
        t0 = time.perf_counter(); fn(); eng.sync(); ts.append(time.perf_counter() - t0)
    return 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts)


def numpy_summary(sf, eng, s):
    fr = eng.smoke_get_frame(s, ('v', 'q'))
    v, q = fr['v'][:, sf.lower_y + 1:sf.higher_y].astype(np.float64), fr['q'][:, sf.lower_y + 1:sf.higher_y].astype(np.float64)
    ok = np.isfinite(v).all(-1) & np.isfinite(q).all(-1)
    return dict(n_nonfinite=int((~ok).sum()), v_max=np.abs(v[ok]).max(), kinetic=0.5 * (v[ok] ** 2).sum(), q_min=q[ok].min(0), q_max=q[ok].max(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--res', type=int, default=128)
    args = ap.parse_args()
    env = make('Circulation-v0', seed=0, loss=True, res=args.res, horizon=10, solver_iters=10)
    te = env.taichi_env
    sim, sf, loss, eng = te.simulator, te.smoke_field, te.loss, te.simulator.engine
    env.reset()
    for _ in range(2):
        env.step(np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.02, 0.04]))
    s = sim.cur_step_local
    rows = [('_get_obs()         existing: get_state_RL, five fields whole', env._get_obs),
            ('loss.step()        existing: q_at, q whole to the host', loss.step),
            ('loss.step_grad()   existing: q_at + add_q_grad_at, dense field up', loss.step_grad),
            ('numpy summary      existing: fe_smoke_get_frame v, q + numpy', lambda: numpy_summary(sf, eng, s))]
    res = [timed(eng, fn) for _, fn in rows]
    obs_host = env._get_obs()
    env.enable_device_obs()
    env.enable_device_loss()
    assert np.array_equal(obs_host, env._get_obs())
    dev = [(f'_get_obs()         device: fe_smoke_cells_get, {eng._smoke_n(env.OBS_LIST)} cells', env._get_obs),
           (f'loss.step()        device: fe_smoke_loss_step, {loss.detector_array_N} detectors', loss.step),
           ('loss.step_grad()   device: fe_smoke_loss_step_grad', loss.step_grad),
           ('smoke_summary()    device: fe_smoke_summary', te.smoke_summary)]
    res_dev = [timed(eng, fn) for _, fn in dev]
    lines = [f'commit {args.commit}', f'backend {eng.elib.backend}, Circulation-v0, smoke grid {sf.n_grid}^3, q_dim {sf.q_dim}, slab {sf.lower_y} < j < {sf.higher_y}, frame {s}',
             'microseconds per call, wall clock with the stream drained before and after: median (min .. max) of 30 after 3 warm-up calls']
    for (name, _), (med, lo, hi), (dname, _), (dmed, dlo, dhi) in zip(rows, res, dev, res_dev):
        lines.append(f'  {name:66s} {med:10.1f}   ({lo:.1f} .. {hi:.1f})')
        lines.append(f'  {dname:66s} {dmed:10.1f}   ({dlo:.1f} .. {dhi:.1f})   x{med / dmed:.1f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
