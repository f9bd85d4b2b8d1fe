"""PNGs of a random-action rollout of one environment, drawn by the headless HIP renderer (renderer_type='HIP').
usage: python scripts/render_rollout.py --env LatteArt-v0 --steps 20 --out DIR [--res W H] [--seed N] [--every K] [--scene] [--surface] [env arguments as name=value ...]
--scene draws the colliders and the smoke field as well (FluidEnv.enable_scene_render), --surface the liquids as one smoothed, translucent surface
(FluidEnv.enable_liquid_surface).  Extra name=value arguments go to the environment's constructor (quality=0.5 n_pool=300 ...)."""
import argparse
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd.envs import make  # noqa: E402
from fluidlab_amd.utils.image import write_png  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--env', required=True)
    ap.add_argument('--steps', type=int, required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--res', type=int, nargs=2, default=None, metavar=('W', 'H'))
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--every', type=int, default=1, help='write every K-th step')
    ap.add_argument('--scene', action='store_true', help='draw the SDF colliders and the smoke field as well')
    ap.add_argument('--surface', action='store_true', help='draw the liquid particles as one smoothed, translucent surface')
    ap.add_argument('env_args', nargs='*', help='name=value arguments of the environment')
    args = ap.parse_args()
    kw = {}
    for item in args.env_args:
        k, v = item.split('=', 1)
        try:
            kw[k] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            kw[k] = v
    kw.setdefault('horizon', max(args.steps, 1))
    env = make(args.env, seed=args.seed, loss=False, renderer_type='HIP', **kw)
    te = env.taichi_env
    if args.res is not None:                                     # the scene's camera at another size
        r = te.renderer
        scale = args.res[1] / r.res[1]
        r.res = (int(args.res[0]), int(args.res[1]))
        r.camera.width, r.camera.height = r.res
        r.camera.focal = r.camera.focal * scale
        te.simulator.engine.render_setup(r.camera, r.lights)
    if args.scene:
        env.enable_scene_render()
    if args.surface:
        env.enable_liquid_surface()
    os.makedirs(args.out, exist_ok=True)
    env.reset()
    rng = np.random.RandomState(args.seed)
    write_png(os.path.join(args.out, '0000.png'), env.render('rgb_array'))
    n = 1
    for i in range(args.steps):
        lo, hi = env.action_range
        action = rng.uniform(lo, hi, env.action_space.shape) if env.action_space is not None else None
        te.step(action)                                          # (loss=False: no reward to ask FluidEnv.step for)
        if (i + 1) % args.every == 0:
            write_png(os.path.join(args.out, f'{i + 1:04d}.png'), env.render('rgb_array'))
            n += 1
    print(f'{n} frames of {args.env} written to {args.out} ({te.renderer.res[0]} x {te.renderer.res[1]})')


if __name__ == '__main__':
    main()
