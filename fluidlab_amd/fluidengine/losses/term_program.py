"""Loss-term programs: a task loss written as a short list of terms the engine evaluates on a GPU-resident frame
(include/fluidengine_ext.h: fe_task_loss_*; kernels in csrc/fe_task_loss.h).  `Sel` and `Term` mirror FeLossSel / FeLossTerm;
`eval_terms_numpy` is a plain fp64 numpy interpreter of the same semantics, with the pairs formed by brute force -- the
restatement the kernels are tested against, independent of host_loss.pairwise_l1."""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from fluidlab_amd import _capi

L1_CONST, SQ_CONST, L1_REF, PAIR_L1 = _capi.FE_TERM_L1_CONST, _capi.FE_TERM_SQ_CONST, _capi.FE_TERM_L1_REF, _capi.FE_TERM_PAIR_L1
AXIS_X, AXIS_Y, AXIS_Z, AXIS_ALL = 1, 2, 4, 7


@dataclass
class Sel:
    """particles with pid in [pid_lo, pid_hi), of material mat (-1: any) and, with require_used, with used[f, p] != 0"""
    pid_lo: int
    pid_hi: int
    mat: int = -1
    require_used: bool = False

    def to_c(self):
        return _capi.FeLossSel(int(self.pid_lo), int(self.pid_hi), int(self.mat), 1 if self.require_used else 0)

    def mask(self, used, mat):
        n = len(used)
        pid = np.arange(n)
        m = (pid >= self.pid_lo) & (pid < self.pid_hi)
        if self.mat >= 0:
            m &= np.asarray(mat) == self.mat
        if self.require_used:
            m &= np.asarray(used) != 0
        return m


@dataclass
class Term:
    """kind, axis_mask (bits 0..2 = x, y, z), selection a, for PAIR_L1 selection b (None: all ordered pairs of a with itself),
    the constant c of L1_CONST / SQ_CONST, and the weight: every constant factor of the term, sign included"""
    kind: int
    axis_mask: int
    a: Sel
    b: Optional[Sel] = None
    c: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    weight: float = 1.0
    name: str = field(default='', compare=False)

    def to_c(self):
        t = _capi.FeLossTerm()
        t.kind, t.axis_mask, t.a = int(self.kind), int(self.axis_mask), self.a.to_c()
        t.b = self.b.to_c() if self.b is not None else _capi.FeLossSel(-1, -1, -1, 0)
        t.c[:] = [float(v) for v in self.c]
        t.weight = float(self.weight)
        return t


def _axes(mask):
    return [a for a in range(3) if (mask >> a) & 1]


def eval_terms_numpy(terms, x, used, mat, ref=None, want_grad=False):
    """values [n_terms] (fp64) of the program on one frame and, with want_grad, d sum_t value_t / d x as [N, 3] fp64 (else None).
    x [N, 3], used [N], mat [N] by particle id; ref [N, 3] for L1_REF.  |d|' = sign(d), 0 at d == 0; the gradient of a particle is
    summed over the terms in their order."""
    x = np.asarray(x, np.float64)
    values = np.zeros((len(terms),), np.float64)
    grad = np.zeros_like(x) if want_grad else None
    for t, T in enumerate(terms):
        ia = np.nonzero(T.a.mask(used, mat))[0]
        if T.kind in (L1_CONST, SQ_CONST, L1_REF):
            total = 0.0
            for a in _axes(T.axis_mask):
                if T.kind == L1_REF:
                    assert ref is not None, 'L1_REF needs ref'
                    d = x[ia, a] - np.asarray(ref, np.float64)[ia, a]
                else:
                    d = x[ia, a] - float(T.c[a])
                total += float((d * d).sum()) if T.kind == SQ_CONST else float(np.abs(d).sum())
                if want_grad:
                    grad[ia, a] += (2.0 * d if T.kind == SQ_CONST else np.sign(d)) * T.weight
            values[t] = T.weight * total
        elif T.kind == PAIR_L1:
            self_pairs = T.b is None
            ib = ia if self_pairs else np.nonzero(T.b.mask(used, mat))[0]
            total = 0.0
            for a in _axes(T.axis_mask):
                d = x[ia, a][:, None] - x[ib, a][None, :]          # every pair
                total += float(np.abs(d).sum())
                if want_grad:
                    sg = np.sign(d)
                    if self_pairs:
                        grad[ia, a] += T.weight * (2.0 * sg.sum(axis=1))
                    else:
                        grad[ia, a] += T.weight * sg.sum(axis=1)
                        grad[ib, a] += T.weight * (-sg.sum(axis=0))
            values[t] = T.weight * total
        else:
            raise ValueError(f'unknown term kind {T.kind}')
    return values, grad
