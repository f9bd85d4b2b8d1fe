"""Cost of the observation fields (include/fluidengine_ext.h: fe_field_obs_*) on the benchmark block (WaterBlock-v0: 128^3, 200k particles)
and on Mixing-v0 as shipped: fe_field_obs_get_dev and fe_field_obs_add_grad_dev for top-down fields of 32 x 1 x 32 and 64 x 1 x 64 cells
with one and four channels and for 32^3 cells with four, over the box of the used particles, on both roads of the scatter (option
field_obs_lds 1: per-workgroup LDS copies, where the channels fit; 0: global atomics).  Beside them, in the same run:
  - fe_obs_get_dev / fe_obs_add_grad_dev with the environment's particle list (the observation the fields stand beside);
  - a torch restatement on the same GPU: the 27 stencil offsets, fp64 index_add_ per channel (forward only);
  - with Mixing-v0: one closed-loop step forward and backward on the device road, with the field observation (64 x 1 x 64, four channels,
    per liquid material, no particle rows) against the particle observation.
Wall clock per call with the engine's stream (and torch's) drained before the clock starts and again before it stops; 5 warm-up calls, then
the median of 30.
usage: python scripts/field_obs_cost.py [--commit TEXT] [--out FILE] [--small] [--only WaterBlock-v0|Mixing-v0]
  --small   reduced scenes (4,096 and 2,592 particles): a dry run of the script, and the figures of profiles/field_obs_cost_small.txt"""
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
from fluidlab_amd.fluidengine.losses.term_program import DensityField  # noqa: E402
from fluidlab_amd.optimizer.closed_loop import ClosedLoopSolver, ObsPolicy  # noqa: E402

SHAPES = [((32, 1, 32), 1), ((32, 1, 32), 4), ((64, 1, 64), 1), ((64, 1, 64), 4), ((32, 32, 32), 4)]


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


def torch_field(x, v, spec, channels):
    """the restatement: fp64 weights, one index_add_ per stencil offset and channel; [channels, cells] float64"""
    import torch
    n = [int(q) for q in spec.n]
    cells = n[0] * n[1] * n[2]
    x = x.double()
    base, w = [], []
    for a in range(3):
        if n[a] == 1:
            base.append(torch.zeros(x.shape[0], dtype=torch.int64, device=x.device))
            w.append(torch.stack([torch.ones_like(x[:, a]), torch.zeros_like(x[:, a]), torch.zeros_like(x[:, a])]))
            continue
        s = (x[:, a] - spec.origin[a]) / spec.cell[a] - 0.5
        b = torch.floor(s - 0.5)
        t = s - b
        base.append(b.long())
        w.append(torch.stack([0.5 * (1.5 - t) ** 2, 0.75 - (t - 1.0) ** 2, 0.5 * (t - 0.5) ** 2]))
    out = torch.zeros((channels, cells), dtype=torch.float64, device=x.device)
    vd = v.double()
    for i in range(3):
        for j in range(3):
            for k in range(3):
                ci, cj, ck = base[0] + i, base[1] + j, base[2] + k
                ok = (ci >= 0) & (ci < n[0]) & (cj >= 0) & (cj < n[1]) & (ck >= 0) & (ck < n[2])
                idx = torch.where(ok, (ci * n[1] + cj) * n[2] + ck, torch.zeros_like(ci))
                wt = torch.where(ok, w[0][i] * w[1][j] * w[2][k], torch.zeros_like(w[0][i]))
                out[0].index_add_(0, idx, wt)
                for c in range(1, channels):
                    out[c].index_add_(0, idx, wt * vd[:, c - 1])
    return out


def fields_alone(name, lib, emit, make_kw):
    import torch
    env = make(name, engine_lib=lib, **make_kw)
    env.enable_device_obs()
    te = env.taichi_env
    sim = te.simulator
    eng = sim.engine
    te.step(None if te.agent is None else np.zeros(te.agent.action_dim))
    f, N, n_list = sim.cur_substep_local, sim.n_particles, eng.n_obs
    dev = torch.device('cuda', eng.device)
    x = torch.empty((N, 3), dtype=torch.float32, device=dev); v = torch.empty_like(x); used = torch.empty((N,), dtype=torch.int32, device=dev)
    eng.get_frame_dev(f, x=x, v=v, used=used)
    keep = used != 0
    xs, vs = x[keep].contiguous(), v[keep].contiguous()
    lo, hi = xs.min(dim=0).values.cpu().numpy().astype(np.float64), xs.max(dim=0).values.cpu().numpy().astype(np.float64)
    limit = torch.cuda.get_device_properties(dev).shared_memory_per_block if hasattr(torch.cuda.get_device_properties(dev), 'shared_memory_per_block') else None

    def sync():
        eng.sync(); torch.cuda.synchronize(dev)
    emit(f'{name} (n_grid {sim.n_grid}, N {N}, {int(keep.sum())} used), frame {f}; fields over the used particles\' box:')
    ox, ov, ou = torch.empty((n_list, 3), dtype=torch.float32, device=dev), torch.empty((n_list, 3), dtype=torch.float32, device=dev), torch.empty((n_list,), dtype=torch.int32, device=dev)
    gx, gv = torch.randn((n_list, 3), device=dev), torch.randn((n_list, 3), device=dev)
    eng.reset_grad()
    emit(f'  fe_obs_get_dev ({n_list} rows)                          {fmt(timed(sync, lambda: eng.get_obs_dev(f, ox, ov, ou)))}')
    emit(f'  fe_obs_add_grad_dev ({n_list} rows)                     {fmt(timed(sync, lambda: eng.obs_add_grad_dev(f, gx, gv)))}')
    for n, channels in SHAPES:
        cell = tuple(float((hi[a] - lo[a]) / n[a]) if n[a] > 1 else 1.0 for a in range(3))
        spec = DensityField(tuple(float(lo[a]) if n[a] > 1 else 0.0 for a in range(3)), cell, n)
        eng.field_obs_set(0, spec, None, channels)
        out = torch.empty((channels,) + n, dtype=torch.float32, device=dev)
        G = torch.randn((channels,) + n, device=dev)
        bytes_lds = channels * 8 * int(np.prod(n))
        row = f'  {n[0]:2d} x {n[1]:2d} x {n[2]:2d} C={channels} ({bytes_lds // 1024:4d} KiB of words)'
        ref = None
        for lds in (1, 0):
            eng.set_option('field_obs_lds', lds)
            t = timed(sync, lambda: eng.field_obs_dev(f, 0, out))
            road = 'LDS road   ' if lds else 'global road'
            if ref is None:
                ref = out.clone()
            same = bool((out == ref).all())
            emit(f'{row}  fe_field_obs_get_dev, field_obs_lds {lds} ({road}){"" if same else " DIFFERS"}  {fmt(t)}')
        eng.set_option('field_obs_lds', -1)
        emit(f'{row}  fe_field_obs_add_grad_dev                          {fmt(timed(sync, lambda: eng.field_obs_add_grad(f, 0, G)))}')
        tt = timed(sync, lambda: torch_field(xs, vs, spec, channels))
        err = float((torch_field(xs, vs, spec, channels).reshape(out.shape) - ref.double()).abs().max())
        emit(f'{row}  torch restatement (27 x fp64 index_add_ per channel)  {fmt(tt)}   max |torch - engine| {err:.3e}')
    if limit is not None:
        emit(f'  (LDS per workgroup as torch reports it: {limit} B; a field takes the LDS road when its words fit the limit the engine reads from the device)')
    eng.close()


def closed_loop_step(name, lib, fields, emit, make_kw):
    import torch
    env = make(name, seed=0, loss=True, engine_lib=lib, ckpt_dest='cpu', **make_kw)
    env.enable_device_obs()
    te = env.taichi_env
    sim = te.simulator
    if fields:
        env.enable_field_obs(env.boundary_fields(fields), particles=False)     # (what run.py --closed_loop --field_obs N observes, without the particle rows)
    pol = ObsPolicy(env, hidden=64, use_agent_state=True, seed=1)
    sol = ClosedLoopSolver(env, pol)
    assert sol._device_road()
    te.set_state(te.get_state()['state'], grad_enabled=True)
    kept = {}

    def sync():
        sim.engine.sync()
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

    forward()
    te.loss.temporal_range = [0, 1]
    te.get_final_loss(); te.reset_grad(); te.get_final_loss_grad()
    backward()
    fw, bw = [], []
    for k in range(35):
        sync(); t0 = time.perf_counter(); forward(); sync(); t1 = time.perf_counter()
        backward(); sync(); t2 = time.perf_counter()
        if k >= 5:
            fw.append(t1 - t0); bw.append(t2 - t1)
    us = lambda ts: (1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts))
    what = f'fields {fields} x 1 x {fields} C=4 per material' if fields else 'particle rows'
    emit(f'  {name:12s} N {sim.n_particles:7d} obs {env.obs_layout()["size"]:6d} ({what})  forward {fmt(us(fw))}   backward {fmt(us(bw))}')
    sim.engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--only', default='', choices=('', 'WaterBlock-v0', 'Mixing-v0'))
    args = ap.parse_args()
    import torch
    lines = []

    def emit(text):
        lines.append(text)
        print(text, flush=True)
    lib = _capi.load_hip()
    stamp = _capi.HIP_LIB_PATH + '.srchash'
    emit(f'commit {args.commit}; build {open(stamp).read().strip()[:16] if os.path.exists(stamp) else "(no source hash beside the library)"}; device {torch.cuda.get_device_name(0)}')
    if args.small:
        emit('reduced scenes (--small)')
    emit(f'backend {lib.backend}; microseconds per call, wall clock, streams drained before and after: median (min .. max) of 30 after 5 warm-up calls')
    block_kw = dict(horizon=2, quality=0.5, n_particles=4096) if args.small else dict(horizon=2)
    mixing_kw = dict(quality=0.5, particle_density=3e4, horizon=12) if args.small else {}
    if args.only in ('', 'WaterBlock-v0'):
        fields_alone('WaterBlock-v0', lib, emit, block_kw)
    if args.only in ('', 'Mixing-v0'):
        fields_alone('Mixing-v0', lib, emit, dict(seed=0, loss=True, ckpt_dest='cpu', **mixing_kw))
        emit('one closed-loop step on the device road (ObsPolicy hidden 64, use_agent_state=True):')
        for fields in (64, 0):
            closed_loop_step('Mixing-v0', lib, fields, emit, mixing_kw)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
