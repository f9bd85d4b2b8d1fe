"""Cost of a picture with the scene in it (include/fluidengine_ext.h: fe_render_scene_frame + fe_render_get of the RGBA image), beside
fe_render_frame + fe_render_get of the same frame:
  - Circulation-v0 at its shipped size (128^3 smoke grid, the room at res 128, 1280 x 1280) after a few steps of the demo policy: smoke alone,
    the room alone, both; and beside one fe_smoke_step of the same build;
  - the benchmark block (128^3 grid, 200k water particles) with one res-128 static (a sphere) at 960 x 960.
march_step and bisect_iters at their defaults.  Wall clock per call with the engine's stream drained before and after; 3 warm-up calls, then
the median of 30.
usage: python scripts/render_scene_cost.py [--commit TEXT] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd import _capi, scenes as S  # noqa: E402
from fluidlab_amd.envs import make  # noqa: E402
from fluidlab_amd.fluidengine.renderers import hip_renderer as HR  # noqa: E402


def timed(eng, fn, warm=3, n=30):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        eng.sync()
        t0 = time.perf_counter(); fn(); eng.sync(); ts.append(time.perf_counter() - t0)
    return 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts)


def row(label, t, base=None, what=''):
    tail = f'   {t[0] / base:.2f} x {what}' if base else ''
    return f'  {label:72s} {t[0]:10.1f}   ({t[1]:.1f} .. {t[2]:.1f}){tail}'


def circulation(lines):
    env = make('Circulation-v0', seed=0, loss=False, renderer_type='HIP')
    te = env.taichi_env
    sim, r, eng = te.simulator, te.renderer, te.simulator.engine
    pol = env.demo_policy()
    te.apply_agent_action_p(pol.get_actions_p())
    for i in range(5):
        te.step(pol.get_action_v(i))
    f, s = sim.cur_substep_local, sim.cur_step_local
    lines.append(f'Circulation-v0 as shipped: smoke grid {te.smoke_field.n_grid}^3, slab {te.smoke_field.lower_y} < j < {te.smoke_field.higher_y}, room SDF at res '
                 f'{te.statics[0].sdf_voxels_res}, image {r.res[0]} x {r.res[1]}, after 5 steps of the demo policy')

    def plain():
        eng.render_frame(f)
        return eng.render_get()[0]

    def scene():
        eng.render_scene_frame(f, s)
        return eng.render_get()[0]

    base = timed(eng, plain)
    lines.append(row('fe_render_frame + fe_render_get (ten parked particles: a blank image)', base))
    step = timed(eng, lambda: eng.smoke_step(s, f))
    lines.append(row('fe_smoke_step (one step of the field the picture shows)', step))
    for label, kw in (('smoke alone', dict(statics=False, effectors=False)), ('the room alone', dict(smoke=False)), ('smoke and the room', {})):
        r.enable_scene(**kw)
        covered = int((scene()[..., :3] != 255).any(-1).sum())
        t = timed(eng, scene)
        enq = timed(eng, lambda: eng.render_scene_frame(f, s))
        note = '   MORE than the smoke step it shows' if t[0] > step[0] else ''
        lines.append(row(f'fe_render_scene_frame + fe_render_get, {label} ({covered} pixels covered)', t, base[0], 'the plain picture') + f', {t[0] / step[0]:.2f} x the smoke step{note}')
        lines.append(row(f'fe_render_scene_frame alone, {label}', enq))
    eng.close()


def block(lines):
    elib = _capi.load_hip()
    sc = S.water_block(n_grid=128, n_particles=200000, seed=0)
    g = np.linspace(0.0, 1.0, 128)
    X, Y, Z = np.meshgrid(g, g, g, indexing='ij')
    vox = (np.sqrt((X - 0.7) ** 2 + (Y - 0.3) ** 2 + (Z - 0.5) ** 2) - 0.15).astype(np.float32)
    T = np.diag([127.0, 127.0, 127.0, 1.0])
    sc['statics'] = [dict(voxels=vox, T=T, friction=0.0)]
    eng = S.make_engine(elib, sc, max_substeps_local=8)
    N, res = sc['N'], (960, 960)
    eng.render_setup(HR.make_camera(res, (0.5, 2.5, 3.5), (0.5, 0.5, 0.5), 30), HR.make_lights(list(HR.DEFAULT_LIGHTS)))
    eng.render_set_colors(np.tile(np.array([[60, 120, 230, 255]], np.uint8), (N, 1)), 0.0075)
    lines.append(f'the benchmark block: 128^3 grid, {N} particles at rest, one static (a sphere of radius 0.15) at res 128 over the unit cube, image {res[0]} x {res[1]}')

    def plain():
        eng.render_frame(0)
        return eng.render_get()[0]

    def scene():
        eng.render_scene_frame(0, 0)
        return eng.render_get()[0]

    base = timed(eng, plain)
    lines.append(row('fe_render_frame + fe_render_get', base))
    eng.render_set_volume(0, _capi.FE_RENDER_VOL_STATIC, 0, (230, 230, 230, 255))
    covered = int((scene()[..., :3] != 255).any(-1).sum())
    lines.append(row(f'fe_render_scene_frame + fe_render_get, the static ({covered} pixels covered)', timed(eng, scene), base[0], 'the plain picture'))
    lines.append(row('fe_render_scene_frame alone', timed(eng, lambda: eng.render_scene_frame(0, 0))))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = [f'commit {args.commit}', f'backend {_capi.load_hip().backend}; march_step 0.5, bisect_iters 10',
             'microseconds per call, wall clock with the stream drained before and after: median (min .. max) of 30 after 3 warm-up calls']
    circulation(lines)
    block(lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
