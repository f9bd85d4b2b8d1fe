"""Cost of a picture with the liquids drawn as a smoothed, translucent surface (include/fluidengine_ext.h: fe_surface_frame + fe_render_get of the
RGBA image), beside fe_render_scene_frame + fe_render_get of the same frame:
  - the benchmark block (128^3 grid, 200k water particles, every particle liquid) at 960 x 960;
  - LatteArt-v0 as shipped (its own camera and size) after a few steps of a constant action, every particle liquid.
The surface's parameters are HIPRenderer.enable_liquid_surface's defaults.  Wall clock per call with the engine's stream drained before and
after; 3 warm-up calls, then the median of 30.  --once draws each surface picture a few times and times nothing: the run to put under
`rocprofv3 --kernel-trace --stats` for the per-kernel split.
usage: python scripts/surface_cost.py [--commit TEXT] [--out FILE] [--once]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from render_scene_cost import row, timed  # noqa: E402
from fluidlab_amd import _capi, scenes as S  # noqa: E402
from fluidlab_amd.envs import make  # noqa: E402
from fluidlab_amd.fluidengine.renderers import hip_renderer as HR  # noqa: E402


def surface_params(radius):
    p = _capi.FeSurfaceParams()
    for k, v in HR.LIQUID_SURFACE_DEFAULTS.items():
        setattr(p, k, v)
    p.range = 4.0 * p.radius_scale * radius
    return p


def measure(lines, eng, f, s, once):
    def scene():
        eng.render_scene_frame(f, s)
        return eng.render_get()[0]

    def surface():
        eng.surface_frame(f, s)
        return eng.render_get()[0]

    if once:
        for _ in range(5):
            surface()
        return
    base = timed(eng, scene)
    lines.append(row('fe_render_scene_frame + fe_render_get (opaque spheres)', base))
    liquid = int(np.isfinite(eng.surface_get()[0]).sum()) if surface() is not None else 0
    lines.append(row(f'fe_surface_frame + fe_render_get ({liquid} pixels of liquid)', timed(eng, surface), base[0], 'the sphere picture'))
    lines.append(row('fe_surface_frame alone (enqueue, then the stream drained)', timed(eng, lambda: eng.surface_frame(f, s))))


def block(lines, once):
    elib = _capi.load_hip()
    sc = S.water_block(n_grid=128, n_particles=200000, seed=0)
    eng = S.make_engine(elib, sc, max_substeps_local=8)
    N, res, radius = sc['N'], (960, 960), 0.0075
    eng.render_setup(HR.make_camera(res, (0.5, 2.5, 3.5), (0.5, 0.5, 0.5), 30), HR.make_lights(list(HR.DEFAULT_LIGHTS)))
    eng.render_set_colors(np.tile(np.array([[60, 120, 230, 255]], np.uint8), (N, 1)), radius)
    eng.surface_set(np.ones(N, np.uint8), surface_params(radius))
    lines.append(f'the benchmark block: 128^3 grid, {N} particles at rest, all liquid, image {res[0]} x {res[1]}')
    measure(lines, eng, 0, 0, once)
    eng.close()


def latteart(lines, once):
    env = make('LatteArt-v0', seed=0, loss=False, renderer_type='HIP')
    te = env.taichi_env
    sim, r, eng = te.simulator, te.renderer, te.simulator.engine
    env.reset()
    action = np.full(env.action_space.shape, 0.004, np.float32)
    for _ in range(5):
        te.step(action)
    env.enable_liquid_surface()
    lines.append(f'LatteArt-v0 as shipped: {sim.n_particles} particles ({int(r.surface_selection.sum())} liquid), image {r.res[0]} x {r.res[1]}, after 5 steps')
    measure(lines, eng, sim.cur_substep_local, 0, once)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--once', action='store_true', help='draw a few surface pictures and time nothing (the run to profile)')
    args = ap.parse_args()
    d = HR.LIQUID_SURFACE_DEFAULTS
    lines = [f'commit {args.commit}', f'backend {_capi.load_hip().backend}; surface defaults: ' + ', '.join(f'{k} {v}' for k, v in d.items()) + ' (range 0: four liquid radii)',
             'microseconds per call, wall clock with the stream drained before and after: median (min .. max) of 30 after 3 warm-up calls']
    block(lines, args.once)
    latteart(lines, args.once)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out and not args.once:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
