"""Cost of one density-loss step at the shipped size of LatteArt-v0 (64^3 grid, particle_density 1e6, 60,000 pool particles): the
FE_TERM_DENSITY_SQ term of the engine's loss-term programs (include/fluidengine_ext.h; kernels in csrc/fe_density.h) on the LDS road and on
the global road of k_density_scatter (option density_lds 1 / 0) and with the engine's own choice (-1), against a torch restatement on the
same frame: the positions downloaded into torch on the device (fe_get_frame_dev), weights in fp64, the field by fp64 index_add_, the
gradient by a gather of the residual.  Two fields: the environment's 64 x 1 x 64 top-down field of the milk, and a 64^3 field over the
cup (262,144 cells: above the LDS cap, so only the global road exists).  The environment is rolled out with its scripted pour first.
Wall clock per call with the engine's stream drained before the clock starts and again before it stops; 5 warm-up calls, then the median of 30.
usage: python scripts/density_loss_cost.py [--commit TEXT] [--out FILE] [--steps N]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd import _capi  # noqa: E402
from fluidlab_amd.configs.macros import MILK  # noqa: E402
from fluidlab_amd.envs import make  # noqa: E402
from fluidlab_amd.fluidengine.losses.term_program import AXIS_ALL, DENSITY_SQ, DensityField, Sel, Term, density_of_points  # noqa: E402


def timed(sync, fn, warm=5, n=30):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        sync()
        t0 = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t0)
    return 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts)


class TorchDensity:
    """the same term in torch on the engine's GPU: fp64 weights, index_add_ for the field, a gather of the residual for the gradient"""

    def __init__(self, eng, spec, target, mat, matching_mat, weight):
        import torch
        self.t, self.eng, self.spec, self.weight = torch, eng, spec, weight
        self.dev = torch.device('cuda', eng.device)
        self.x = torch.zeros((eng.N, 3), dtype=torch.float32, device=self.dev)
        self.used = torch.zeros((eng.N,), dtype=torch.int32, device=self.dev)
        self.is_mat = torch.as_tensor(np.asarray(mat) == matching_mat, device=self.dev)
        self.target = torch.as_tensor(np.asarray(target, np.float64).reshape(-1), device=self.dev)
        self.g32 = torch.zeros((eng.N, 3), dtype=torch.float32, device=self.dev)

    def _stencil(self, f):
        t = self.t
        self.eng.get_frame_dev(f, x=self.x, used=self.used)
        idx = t.nonzero((self.used > 0) & self.is_mat, as_tuple=False)[:, 0]
        x = self.x[idx].to(t.float64)
        base, w, dw = [], [], []
        for a in range(3):
            if self.spec.n[a] == 1:
                base.append(t.zeros(len(idx), dtype=t.int64, device=self.dev))
                one, zero = t.ones(len(idx), dtype=t.float64, device=self.dev), t.zeros(len(idx), dtype=t.float64, device=self.dev)
                w.append([one, zero, zero]); dw.append([zero, zero, zero])
                continue
            s = (x[:, a] - self.spec.origin[a]) / self.spec.cell[a] - 0.5
            b = t.floor(s - 0.5)
            tt = s - b
            base.append(b.to(t.int64))
            w.append([0.5 * (1.5 - tt) ** 2, 0.75 - (tt - 1.0) ** 2, 0.5 * (tt - 0.5) ** 2])
            dw.append([-(1.5 - tt) / self.spec.cell[a], -2.0 * (tt - 1.0) / self.spec.cell[a], (tt - 0.5) / self.spec.cell[a]])
        return idx, base, w, dw

    def _cells(self, base):
        n = self.spec.n
        for i in range(3 if n[0] > 1 else 1):
            for j in range(3 if n[1] > 1 else 1):
                for k in range(3 if n[2] > 1 else 1):
                    ci, cj, ck = base[0] + i, base[1] + j, base[2] + k
                    ok = (ci >= 0) & (ci < n[0]) & (cj >= 0) & (cj < n[1]) & (ck >= 0) & (ck < n[2])
                    yield i, j, k, ok, ((ci * n[1] + cj) * n[2] + ck).clamp(0, int(np.prod(n)) - 1)

    def _resid(self, base, w):
        t = self.t
        D = t.zeros(int(np.prod(self.spec.n)), dtype=t.float64, device=self.dev)
        for i, j, k, ok, cell in self._cells(base):
            D.index_add_(0, cell, t.where(ok, w[0][i] * w[1][j] * w[2][k], t.zeros_like(w[0][i])))
        return D - self.target

    def forward(self, f):
        _, base, w, _ = self._stencil(f)
        r = self._resid(base, w)
        return float(self.weight * (r * r).sum())               # (the value reaches the host, as HostLoss's torch path has it)

    def backward(self, f):
        t = self.t
        idx, base, w, dw = self._stencil(f)
        r = 2.0 * self.weight * self._resid(base, w)
        g = t.zeros((len(idx), 3), dtype=t.float64, device=self.dev)
        for i, j, k, ok, cell in self._cells(base):
            rc = t.where(ok, r[cell], t.zeros_like(r[cell]))
            g[:, 0] += rc * dw[0][i] * w[1][j] * w[2][k]
            g[:, 1] += rc * w[0][i] * dw[1][j] * w[2][k]
            g[:, 2] += rc * w[0][i] * w[1][j] * dw[2][k]
        self.g32.zero_()
        self.g32[idx] = g.to(t.float32)
        t.cuda.synchronize(self.dev)                          # the engine reads it on its own stream
        self.eng.add_grad_dev(f, gx=self.g32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--steps', type=int, default=100)
    args = ap.parse_args()
    lines = []

    def emit(text):
        lines.append(text)
        print(text, flush=True)
    emit(f'commit {args.commit}')
    emit('microseconds per call, wall clock, stream drained before and after: median (min .. max) of 30 after 5 warm-up calls')
    env = make('LatteArt-v0', seed=0, loss=True, loss_type='density', horizon=args.steps + 2, horizon_action=args.steps + 2, max_substeps_local=None)
    te = env.taichi_env
    rng = np.random.RandomState(5)
    cloud = np.stack([rng.uniform(0.3, 0.7, 20000), rng.uniform(0.52, 0.9, 20000), rng.uniform(0.35, 0.65, 20000)], axis=1)
    te.loss.set_target_points(cloud)                          # (the rollout evaluates the loss on the host path)
    sim = te.simulator
    eng = sim.engine
    pol = env.demo_policy()
    te.set_state(te.get_state()['state'], grad_enabled=True)
    te.apply_agent_action_p(pol.get_actions_p())
    for i in range(args.steps):
        te.step(pol.get_action_v(i, agent=te.agent, update=True))
    f = sim.cur_substep_local
    N = sim.n_particles
    mat = sim.particles_i.mat.to_numpy()
    x, used = np.zeros((N, 3), np.float32), np.zeros((N,), np.int32)
    eng.get_frame(f, x=x, used=used)
    milk = (used != 0) & (mat == MILK)
    emit(f'LatteArt-v0: backend {eng.elib.backend}, n_grid {sim.n_grid}, N {N}, frame {f} after {args.steps} steps; {int(milk.sum())} used milk particles '
         f'(the selection: pid 0..N, material MILK, used)')
    fields = (('64 x 1 x 64 (the environment\'s field)', env.density_field),
              ('64 x 64 x 64 over the cup', DensityField((0.08, 0.5, 0.08), (0.84 / 64, 0.45 / 64, 0.84 / 64), (64, 64, 64))))
    eng.task_loss_alloc(1)
    sel = Sel(0, N, MILK, True)
    for name, spec in fields:
        cells = int(np.prod(spec.shape))
        target = density_of_points(cloud, spec)
        eng.density_set_field(0, spec)
        eng.density_set_target(0, target)
        eng.task_loss_set_terms([Term(DENSITY_SQ, AXIS_ALL, sel, weight=1.0, field=0)])
        K = density_of_points(x[milk], spec, counts=True)[1]
        emit(f'field {name}: {cells} cells, {int((K > 0).sum())} hit by the milk, {int(K.sum())} deposits'
             + ('' if cells <= _capi.FE_DENSITY_LDS_CELLS else f'; above the LDS cap of {_capi.FE_DENSITY_LDS_CELLS} cells: every setting takes the global road'))
        eng.reset_grad()
        values = {}
        for tag, lds in (('device, global road (density_lds 0)', 0), ('device, LDS road (density_lds 1)', 1), ('device, the engine\'s choice (density_lds -1)', -1)):
            eng.set_option('density_lds', lds)
            fwd = timed(eng.sync, lambda: eng.task_loss_step(0, f))
            bwd = timed(eng.sync, lambda: eng.task_loss_step_grad(0, f, 1.0))
            eng.task_loss_clear()
            eng.task_loss_step(0, f)
            values[tag] = float(eng.task_loss_get(1)[0])
            emit(f'  {tag:46s} forward {fwd[0]:9.1f} ({fwd[1]:.1f} .. {fwd[2]:.1f})   backward {bwd[0]:9.1f} ({bwd[1]:.1f} .. {bwd[2]:.1f})')
        assert len(set(values.values())) == 1, values            # the roads give the same words
        import torch
        td = TorchDensity(eng, spec, target, mat, MILK, 1.0)

        def sync():
            eng.sync()
            torch.cuda.synchronize(td.dev)
        fwd = timed(sync, lambda: td.forward(f))
        bwd = timed(sync, lambda: td.backward(f))
        v_torch = td.forward(f)
        emit(f'  {"torch restatement (fp64 index_add_)":46s} forward {fwd[0]:9.1f} ({fwd[1]:.1f} .. {fwd[2]:.1f})   backward {bwd[0]:9.1f} ({bwd[1]:.1f} .. {bwd[2]:.1f})')
        v_dev = next(iter(values.values()))
        emit(f'  value: device {v_dev!r}, torch {v_torch!r}, relative difference {abs(v_dev - v_torch) / abs(v_torch):.2e}')
        del td
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
