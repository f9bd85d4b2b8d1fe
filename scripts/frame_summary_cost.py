"""Cost of the frame reads that stay on the GPU (include/fluidengine_ext.h) on the benchmark block: 128^3 grid, 200k water particles in
[0.30, 0.53]^3 as two bodies of 100k, through the Python stack (TaichiEnv -> MPMSimulator -> C ABI), after 30 substeps.
  MPMSimulator.get_obs_RL()  (fe_obs_get: the 2 x 200 particles FluidEnv._get_obs keeps)   against   MPMSimulator.get_state_RL()  (fe_get_frame: x, v, used of all N)
  Engine.frame_summary(f)    (fe_frame_summary: two bodies + the whole frame)               against   fe_get_frame(f) of x, v, C, F, used
Wall clock per call, synchronisation included; 5 warm-up calls, then the median of 50.
usage: python scripts/frame_summary_cost.py [--commit TEXT] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd import scenes as S  # noqa: E402
from fluidlab_amd.configs.macros import WATER  # noqa: E402
from fluidlab_amd.fluidengine.taichi_env import TaichiEnv  # noqa: E402


def timed(fn, warm=5, n=50):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lo, mid, hi = 0.30, 0.415, 0.53
    te = TaichiEnv(quality=2, particle_density=100000 / ((mid - lo) * (hi - lo) ** 2), max_substeps_local=50, horizon=10)
    te.add_body(type='cube', lower=(lo, lo, lo), upper=(mid, hi, hi), material=WATER)
    te.add_body(type='cube', lower=(mid, lo, lo), upper=(hi, hi, hi), material=WATER)
    te.build()
    for _ in range(3):
        te.step(None)
    sim = te.simulator
    eng, f, N = sim.engine, sim.cur_substep_local, sim.n_particles
    bodies = te.particles['bodies']
    ids = np.concatenate([np.asarray(bodies['particle_ids'][b])[::max(1, bodies['n_particles'][b] // 200)] for b in range(bodies['n'])])
    sim.set_obs_particles(ids)
    sim.frame_summary(by='body')                               # (sets the groups: the two bodies)
    rows = [(f'MPMSimulator.get_obs_RL()    fe_obs_get, {len(ids)} rows', sim.get_obs_RL),
            ('MPMSimulator.get_state_RL()  fe_get_frame x, v, used [N]', sim.get_state_RL),
            ('Engine.frame_summary(f)      fe_frame_summary, 2 bodies + frame', lambda: eng.frame_summary(f)),
            ('scenes.get_state(eng, f)     fe_get_frame x, v, C, F, used [N]', lambda: S.get_state(eng, f))]
    lines = [f'commit {args.commit}', f'backend {eng.elib.backend}, n_grid {sim.n_grid}, N {N} in {bodies["n"]} bodies, frame {f}',
             'microseconds per call, wall clock with synchronisation: median (min .. max) of 50 after 5 warm-up calls']
    for name, fn in rows:
        med, lo_, hi_ = timed(fn)
        lines.append(f'  {name:66s} {med:10.1f}   ({lo_:.1f} .. {hi_:.1f})')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
