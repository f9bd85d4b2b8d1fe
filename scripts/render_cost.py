"""Cost of a picture from the headless renderer (include/fluidengine_ext.h: fe_render_frame + fe_render_get of the RGBA image) at 960 x 960
on the benchmark's block -- 128^3 grid, 200k water particles -- once at the frame the benchmark starts from and once after the block has
fallen and spread, with option render_lane_pixels at its default, at 0 (every sphere drawn by its whole wave) and at 2^31 - 1 (every sphere by
its own lane).  Beside it: fe_get_frame of x and used alone for the same frame, the least any host-side renderer would have to download
before it could draw a pixel.  Wall clock per call with the engine's stream drained before and after; 3 warm-up calls, then the median of 30.
usage: python scripts/render_cost.py [--commit TEXT] [--out FILE] [--res W H] [--spread-substeps N]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd import _capi, scenes as S  # noqa: E402
from fluidlab_amd.fluidengine.renderers import hip_renderer as HR  # noqa: E402

CHUNK = 100


def timed(eng, fn, warm=3, n=30):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        eng.sync()
        t0 = time.perf_counter(); fn(); eng.sync(); ts.append(time.perf_counter() - t0)
    return 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--res', type=int, nargs=2, default=(960, 960))
    ap.add_argument('--spread-substeps', type=int, default=3000)
    args = ap.parse_args()
    elib = _capi.load_hip()
    sc = S.water_block(n_grid=128, n_particles=200000, seed=0)
    eng = S.make_engine(elib, sc, max_substeps_local=CHUNK)
    N = sc['N']
    radius = 0.0075
    eng.render_setup(HR.make_camera(args.res, (0.5, 2.5, 3.5), (0.5, 0.5, 0.5), 30), HR.make_lights(list(HR.DEFAULT_LIGHTS)))
    eng.render_set_colors(np.tile(np.array([[60, 120, 230, 255]], np.uint8), (N, 1)), radius)
    x, used = np.zeros((N, 3), np.float32), np.zeros((N,), np.int32)
    default = _capi.FE_RENDER_LANE_PIXELS

    def picture():
        eng.render_frame(0)
        return eng.render_get()[0]

    lines = [f'commit {args.commit}',
             f'backend {elib.backend}, water block 128^3 grid, {N} particles, image {args.res[0]} x {args.res[1]}, particle radius {radius}, camera (0.5, 2.5, 3.5) -> (0.5, 0.5, 0.5), fov 30',
             'microseconds per call, wall clock with the stream drained before and after: median (min .. max) of 30 after 3 warm-up calls']
    for label in ('frame 0 (the block at rest, where the benchmark starts)', f'after {args.spread_substeps} substeps (fallen and spread)'):
        covered = int((picture()[..., :3] != 255).any(-1).sum())
        lines.append(f'{label}: {covered} of {args.res[0] * args.res[1]} pixels covered')
        base = timed(eng, lambda: eng.get_frame(0, x=x, used=used))
        lines.append(f'  {"fe_get_frame of x and used (download only, nothing drawn)":66s} {base[0]:10.1f}   ({base[1]:.1f} .. {base[2]:.1f})')
        for name, lp in ((f'default ({default})', default), ('0 (wave road only)', 0), ('2^31 - 1 (lane road only)', 2 ** 31 - 1)):
            eng.set_option('render_lane_pixels', lp)
            med, lo, hi = timed(eng, picture)
            eng.set_option('render_lane_pixels', default)
            lines.append(f'  {"fe_render_frame + fe_render_get, render_lane_pixels " + name:66s} {med:10.1f}   ({lo:.1f} .. {hi:.1f})   {med / base[0]:.2f} x the download')
        enq = timed(eng, lambda: eng.render_frame(0))
        lines.append(f'  {"fe_render_frame alone (clear + splat + shade, nothing copied)":66s} {enq[0]:10.1f}   ({enq[1]:.1f} .. {enq[2]:.1f})')
        if label.startswith('frame 0'):
            for _ in range(args.spread_substeps // CHUNK):
                eng.step(0, 0, CHUNK, 0)
                eng.copy_frame(CHUNK, 0)
            eng.sync()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    eng.close()


if __name__ == '__main__':
    main()
