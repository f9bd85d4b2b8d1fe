"""Cost of one Chamfer loss step -- the FE_TERM_NEAREST_SQ and FE_TERM_COVER_SQ terms of the engine's loss-term programs
(include/fluidengine_ext.h; kernels in csrc/fe_nearest.h) -- forward and backward, on a block of 200,000 particles (the benchmark's size)
against clouds of 10,000 and 100,000 points that overlap the block or lie disjoint from it, with the engine's own grid resolution
(nn_cells 0) and two forced ones, against a torch restatement on the same GPU: the positions downloaded into torch on the device
(fe_get_frame_dev), chunked fp64 torch.cdist + argmin in both directions, the gradient by index_add_ -- the only other road a user has.
Wall clock per call with the engine's stream drained before the clock starts and again before it stops; 5 warm-up calls, then the median of
30 (3 where one call takes longer than 50 ms).
The torch road is measured for the 10,000-point clouds only (the distance matrix of 100,000 x 200,000 is 2 x 10^10 entries).
usage: python scripts/chamfer_loss_cost.py [--out FILE] [--particles N] [--no-torch]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd import _capi  # noqa: E402
from fluidlab_amd.scenes import make_engine, water_block  # noqa: E402
from fluidlab_amd.fluidengine.losses.term_program import AXIS_ALL, AXIS_X, AXIS_Z, COVER_SQ, NEAREST_SQ, Sel, Term  # noqa: E402


def timed(sync, fn, warm=5, n=30):
    sync()
    t0 = time.perf_counter(); fn(); sync()
    if time.perf_counter() - t0 > 0.05:
        warm, n = 1, 3
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        sync()
        t0 = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t0)
    return 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts), n


class TorchChamfer:
    """the two terms in torch on the engine's GPU: chunked fp64 cdist + argmin in both directions, index_add_ for COVER's gradient"""

    def __init__(self, eng, cloud, axes, chunk=4096):
        import torch
        self.t, self.eng, self.axes, self.chunk = torch, eng, axes, chunk
        self.dev = torch.device('cuda', eng.device)
        self.x = torch.zeros((eng.N, 3), dtype=torch.float32, device=self.dev)
        self.used = torch.zeros((eng.N,), dtype=torch.int32, device=self.dev)
        self.cloud = torch.as_tensor(np.asarray(cloud, np.float64)[:, axes], device=self.dev)
        self.g32 = torch.zeros((eng.N, 3), dtype=torch.float32, device=self.dev)

    def _nearest(self, q, c):
        t = self.t
        idx, d2 = [], []
        for lo in range(0, len(q), self.chunk):
            d = t.cdist(q[lo:lo + self.chunk], c) ** 2
            m = d.min(dim=1)
            idx.append(m.indices); d2.append(m.values)
        return t.cat(idx), t.cat(d2)

    def step(self, f, grad):
        t = self.t
        self.eng.get_frame_dev(f, x=self.x, used=self.used)
        sel = t.nonzero(self.used > 0, as_tuple=False)[:, 0]
        x = self.x[sel].to(t.float64)[:, self.axes]
        j, d2p = self._nearest(x, self.cloud)
        p, d2c = self._nearest(self.cloud, x)
        value = d2p.sum() + d2c.sum()
        if grad:
            g = 2.0 * (x - self.cloud[j])
            g.index_add_(0, p, 2.0 * (x[p] - self.cloud))
            full = t.zeros((self.eng.N, 3), dtype=t.float64, device=self.dev)
            full[sel[:, None], t.as_tensor(self.axes, device=self.dev)[None, :]] = g
            self.g32.copy_(full)
            t.cuda.synchronize(self.dev)
            self.eng.add_grad_dev(f, gx=self.g32)
        return value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'chamfer_loss_cost.txt'))
    ap.add_argument('--particles', type=int, default=200000)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    lib = _capi.load_hip()
    N = args.particles
    sc = water_block(n_grid=64, n_particles=N, lo=0.3, hi=0.6)
    eng = make_engine(lib, sc, max_substeps_local=4)
    eng.task_loss_alloc(1)
    sync = eng.sync
    rs = np.random.RandomState(0)
    lines = [f'Chamfer loss step: {N} particles in [0.3, 0.6]^3; us per call, median (min .. max) of n; fwd = fe_task_loss_step, bwd = fe_task_loss_step_grad',
             'both terms (NEAREST + COVER) in one program; torch = chunked fp64 cdist + argmin on the same GPU, the frame fetched with fe_get_frame_dev']
    for mask, mname, axes in ((AXIS_ALL, 'xyz', [0, 1, 2]), (AXIS_X | AXIS_Z, 'x|z', [0, 2])):
        for M in (10000, 100000):
            for where, off in (('overlapping', 0.0), ('disjoint', 0.6)):
                cloud = (0.35 + 0.25 * rs.rand(M, 3) + [off, 0.0, off]).astype(np.float32)
                eng.cloud_set(0, cloud)
                sel = Sel(0, N, -1, True)
                eng.task_loss_set_terms([Term(NEAREST_SQ, mask, sel, cloud=0), Term(COVER_SQ, mask, sel, cloud=0)])
                for cells in (0, 16, 64):
                    eng.set_option('nn_cells', cells)
                    fwd = timed(sync, lambda: eng.task_loss_step(0, 0))
                    bwd = timed(sync, lambda: eng.task_loss_step_grad(0, 0, 1.0))
                    lines.append(f'mask {mname} cloud {M:6d} {where:11s} nn_cells {cells:2d}: fwd {fwd[0]:10.1f} ({fwd[1]:.1f} .. {fwd[2]:.1f}) n {fwd[3]}   '
                                 f'bwd {bwd[0]:10.1f} ({bwd[1]:.1f} .. {bwd[2]:.1f}) n {bwd[3]}')
                    print(lines[-1], flush=True)
                eng.set_option('nn_cells', 0)
                if not args.no_torch and M * N <= 2e9 + 1:
                    tc = TorchChamfer(eng, cloud, axes)
                    fwd = timed(sync, lambda: float(tc.step(0, False)))
                    bwd = timed(sync, lambda: float(tc.step(0, True)))
                    lines.append(f'mask {mname} cloud {M:6d} {where:11s} torch      : fwd {fwd[0]:10.1f} ({fwd[1]:.1f} .. {fwd[2]:.1f}) n {fwd[3]}   '
                                 f'bwd {bwd[0]:10.1f} ({bwd[1]:.1f} .. {bwd[2]:.1f}) n {bwd[3]}')
                    print(lines[-1], flush=True)
                eng.task_loss_set_terms(None)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
