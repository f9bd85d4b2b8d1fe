"""Cost of one SmokeField.step (fe_smoke_step) in Circulation-v0 at its shipped size: 128^3 smoke grid, q_dim 1, slab 60 < j < 68, 50 Jacobi
sweeps, after two steps.  Wall clock per call with the engine's stream drained before and after (10 warm-up calls, then the median of 200),
and per step of ten calls back to back (median of 50).  `--lib` times another build of the engine with the same ABI.
usage: python scripts/smoke_step_cost.py [--lib libfluidengine_hip.so] [--res N]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd import _capi  # noqa: E402


def timed(eng, fn, warm, n):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        eng.sync()
        t0 = time.perf_counter(); fn(); eng.sync(); ts.append(time.perf_counter() - t0)
    return 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None)
    ap.add_argument('--res', type=int, default=128)
    args = ap.parse_args()
    if args.lib:
        _capi.HIP_LIB_PATH = os.path.abspath(args.lib)
    from fluidlab_amd.envs import make
    env = make('Circulation-v0', seed=0, loss=True, res=args.res, horizon=10)
    sim, sf = env.taichi_env.simulator, env.taichi_env.smoke_field
    eng = sim.engine
    env.reset()
    for _ in range(2):
        env.step(np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.02, 0.04]))
    s, f = sim.cur_step_local, sim.cur_substep_local

    def ten():
        for _ in range(10):
            eng.smoke_step(s, f)
    one = timed(eng, lambda: eng.smoke_step(s, f), 10, 200)
    many = [t / 10 for t in timed(eng, ten, 3, 50)]
    print(f'library {os.path.relpath(_capi.HIP_LIB_PATH, ROOT)}, backend {eng.elib.backend}, Circulation-v0, smoke grid {sf.n_grid}^3, q_dim {sf.q_dim}, '
          f'slab {sf.lower_y} < j < {sf.higher_y}, frame {s}')
    print('microseconds, wall clock with the stream drained before and after: median (min .. max)')
    print(f'  fe_smoke_step, one call                 {one[0]:8.1f}   ({one[1]:.1f} .. {one[2]:.1f})')
    print(f'  fe_smoke_step, per step of ten calls    {many[0]:8.1f}   ({many[1]:.1f} .. {many[2]:.1f})')


if __name__ == '__main__':
    main()
