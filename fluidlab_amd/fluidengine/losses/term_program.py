"""Loss-term programs: a task loss written as a short list of terms the engine evaluates on a GPU-resident frame
(include/fluidengine_ext.h: fe_task_loss_*; kernels in csrc/fe_task_loss.h).  `Sel` and `Term` mirror FeLossSel / FeLossTerm;
`eval_terms_numpy` is a plain fp64 numpy interpreter of the same semantics, with the pairs formed by brute force -- the
restatement the kernels are tested against, independent of host_loss.pairwise_l1.  `DensityField` mirrors FeDensitySpec and
`density_of_points` is the brute-force fp64 rasteriser of the density term, without the engine's fixed-point quantisation.
`nearest_bruteforce` is the all-pairs fp64 restatement of the nearest-point search behind NEAREST_SQ / COVER_SQ (csrc/fe_nearest.h)."""
from dataclasses import dataclass, field as _dc_field
from typing import Optional, Tuple

import numpy as np

from fluidlab_amd import _capi

L1_CONST, SQ_CONST, L1_REF, PAIR_L1 = _capi.FE_TERM_L1_CONST, _capi.FE_TERM_SQ_CONST, _capi.FE_TERM_L1_REF, _capi.FE_TERM_PAIR_L1
DENSITY_SQ = _capi.FE_TERM_DENSITY_SQ
NEAREST_SQ, COVER_SQ = _capi.FE_TERM_NEAREST_SQ, _capi.FE_TERM_COVER_SQ
COVER_FIX = 2.0 ** 40                                        # the fixed point of the COVER gradient (FE_NN_FIX)
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
    the constant c of L1_CONST / SQ_CONST, the weight: every constant factor of the term, sign included, for DENSITY_SQ
    (axis_mask AXIS_ALL) the id of the density field, and for NEAREST_SQ / COVER_SQ the id of the target cloud"""
    kind: int
    axis_mask: int
    a: Sel
    b: Optional[Sel] = None
    c: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    weight: float = 1.0
    name: str = _dc_field(default='', compare=False)
    field: int = 0
    cloud: int = 0

    def to_c(self):
        t = _capi.FeLossTerm()
        t.kind, t.axis_mask, t.a = int(self.kind), int(self.axis_mask), self.a.to_c()
        if self.kind == DENSITY_SQ:                          # the field id travels in b.pid_lo, the rest of b is zero
            t.b = _capi.FeLossSel(int(self.field), 0, 0, 0)
        elif self.kind in (NEAREST_SQ, COVER_SQ):            # likewise the cloud id
            t.b = _capi.FeLossSel(int(self.cloud), 0, 0, 0)
        else:
            t.b = self.b.to_c() if self.b is not None else _capi.FeLossSel(-1, -1, -1, 0)
        t.c[:] = [float(v) for v in self.c]
        t.weight = float(self.weight)
        return t


@dataclass
class DensityField:
    """FeDensitySpec: n cells per axis (1 = projected along that axis) of size `cell`, cell (0, 0, 0) with its corner at `origin`;
    cell (i, j, k) has its centre at origin + (i + 0.5, j + 0.5, k + 0.5) cell"""
    origin: Tuple[float, float, float]
    cell: Tuple[float, float, float]
    n: Tuple[int, int, int]

    def to_c(self):
        c = _capi.FeDensitySpec()
        c.origin[:] = [float(v) for v in self.origin]
        c.cell[:] = [float(v) for v in self.cell]
        c.n[:] = [int(v) for v in self.n]
        c.pad = 0
        return c

    @property
    def shape(self):
        return tuple(int(v) for v in self.n)


def _axes(mask):
    return [a for a in range(3) if (mask >> a) & 1]


def fused_middle_weight(d):
    """0.75 - d d with ONE rounding, for fp64 d = t - 1 in [-0.5, 0.5): what the device's fused multiply-add gives for the middle weight of
    the stencil (the compiler contracts fe_dn_axis' 0.75 - (t - 1)(t - 1)).  d d = p + e exactly (Dekker's product), 0.75 - p = s + r
    exactly (two-sum); r and e are multiples of 2^-106 below 2^-53, so r - e is exact and s + (r - e) rounds the exact value once."""
    d = np.asarray(d, np.float64)
    p = d * d
    c = 134217729.0 * d
    hi = c - (c - d)
    lo = d - hi
    e = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo
    s = 0.75 - p
    bb = s - 0.75
    r = (0.75 - (s - bb)) + (-p - bb)
    return s + (r - e)


def density_stencil(x, spec, fused=False):
    """the quadratic B-spline stencil of every point on the field, fp64: (ok [M], base [M, 3] int64, w [M, 3, 3], dw [M, 3, 3]).  On
    axis a point p touches the cells base[p, a] + i, i = 0..2, with weight w[p, a, i] and derivative dw[p, a, i] with respect to x_a; a
    projected axis has base 0 and w = (1, 0, 0), dw = 0.  ok is False for a point that deposits nothing: a non-finite coordinate, or
    |u| > 2^30 on an unprojected axis (its w and dw are zero).  fused: the middle weight with one rounding (fused_middle_weight), the bits
    of the engine's weights."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    M = len(x)
    ok = np.isfinite(x).all(axis=1)
    base = np.zeros((M, 3), np.int64)
    w, dw = np.zeros((M, 3, 3), np.float64), np.zeros((M, 3, 3), np.float64)
    for a in range(3):
        if int(spec.n[a]) == 1:
            w[:, a, 0] = 1.0
            continue
        with np.errstate(invalid='ignore', over='ignore'):
            u = (x[:, a] - float(spec.origin[a])) / float(spec.cell[a])
            ok &= np.abs(u) <= 2.0 ** 30
        u = np.where(ok, u, 0.0)
        s = u - 0.5
        b = np.floor(s - 0.5)
        t = s - b
        base[:, a] = b.astype(np.int64)
        inv = 1.0 / float(spec.cell[a])
        w[:, a, 0], w[:, a, 1], w[:, a, 2] = 0.5 * (1.5 - t) * (1.5 - t), 0.75 - (t - 1.0) * (t - 1.0), 0.5 * (t - 0.5) * (t - 0.5)
        if fused:
            w[:, a, 1] = fused_middle_weight(t - 1.0)
        dw[:, a, 0], dw[:, a, 1], dw[:, a, 2] = -(1.5 - t) * inv, -2.0 * (t - 1.0) * inv, (t - 0.5) * inv
    w[~ok] = 0.0
    dw[~ok] = 0.0
    return ok, base, w, dw


def _stencil_cells(spec, ok, base):
    """for each of the 27 stencil offsets (i, j, k): the points whose cell is inside the field and its linear index (i n1 + j) n2 + k"""
    n = [int(v) for v in spec.n]
    for i in range(3):
        for j in range(3):
            for k in range(3):
                ci, cj, ck = base[:, 0] + i, base[:, 1] + j, base[:, 2] + k
                m = ok & (ci >= 0) & (ci < n[0]) & (cj >= 0) & (cj < n[1]) & (ck >= 0) & (ck < n[2])
                idx = np.nonzero(m)[0]
                yield (i, j, k), idx, ((ci[idx] * n[1] + cj[idx]) * n[2] + ck[idx])


def density_of_points(x, spec, counts=False):
    """the density field of the points x [M, 3], float64 shaped spec.n: every point adds the product over the axes of its weights to the
    cells of its stencil that lie inside the field (brute force over the 27 offsets, no quantisation).  counts=True: also the number of
    deposits per cell (int64, same shape)."""
    n = tuple(int(v) for v in spec.n)
    ok, base, w, _ = density_stencil(x, spec)
    D = np.zeros(int(np.prod(n)), np.float64)
    K = np.zeros(int(np.prod(n)), np.int64)
    for (i, j, k), idx, cell in _stencil_cells(spec, ok, base):
        np.add.at(D, cell, w[idx, 0, i] * w[idx, 1, j] * w[idx, 2, k])
        np.add.at(K, cell, 1)
    return (D.reshape(n), K.reshape(n)) if counts else D.reshape(n)


def density_grad_of_points(x, spec, r):
    """d sum_c r_c D_c / d x for constant r (shaped spec.n): [M, 3] fp64, sum over the in-field stencil cells of r_c d w_pc / d x_a"""
    ok, base, w, dw = density_stencil(x, spec)
    r = np.asarray(r, np.float64).reshape(-1)
    g = np.zeros((len(ok), 3), np.float64)
    for (i, j, k), idx, cell in _stencil_cells(spec, ok, base):
        rc = r[cell]
        g[idx, 0] += rc * dw[idx, 0, i] * w[idx, 1, j] * w[idx, 2, k]
        g[idx, 1] += rc * w[idx, 0, i] * dw[idx, 1, j] * w[idx, 2, k]
        g[idx, 2] += rc * w[idx, 0, i] * w[idx, 1, j] * dw[idx, 2, k]
    return g


FIELD_OBS_DENSITY_FIX = 2.0 ** 40                            # fe_dn_quant: llrint(w 2^40)
FIELD_OBS_MOMENTUM_FIX = 2.0 ** 28                           # fe_fo_quant: llrint(w v_a 2^28)
FIELD_OBS_MAX_V = 2.0 ** 10                                  # |v_a| above it: the particle deposits nothing


def field_obs_ok(x, v, spec, fused=True):
    """(ok [M], base, w, dw): density_stencil with the velocity guard of the observation fields on top -- a point with a non-finite
    velocity word or |v_a| > 2^10 on any axis deposits nothing in any channel and gets no gradient"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    ok, base, w, dw = density_stencil(x, spec, fused=fused)
    with np.errstate(invalid='ignore'):
        ok = ok & np.isfinite(v).all(axis=1) & (np.abs(v) <= FIELD_OBS_MAX_V).all(axis=1)
    return ok, base, w, dw


def field_obs_of_points(x, v, spec, channels=4, quantise=True):
    """the observation field (include/fluidengine_ext.h: fe_field_obs_*) of the points x [M, 3] with velocities v [M, 3]: float64
    [channels, n0, n1, n2], channel 0 the density sum_p w_pc, channels 1..3 the momentum sum_p w_pc v_p,a.  quantise=True: the values the
    engine's words decode to, bit for bit when x and v hold the frame's fp32 words -- the same guards, the weights with the device's
    roundings, every deposit np.rint(w 2^40) / np.rint(w v_a 2^28) summed in int64.  quantise=False: plain fp64 sums."""
    assert channels in (1, 4), 'channels must be 1 or 4'
    n = tuple(int(q) for q in spec.n)
    cells = int(np.prod(n))
    v = np.asarray(v, np.float64).reshape(-1, 3)
    ok, base, w, _ = field_obs_ok(x, v, spec, fused=quantise)
    out = np.zeros((channels, cells), np.int64 if quantise else np.float64)
    for (i, j, k), idx, cell in _stencil_cells(spec, ok, base):
        wt = w[idx, 0, i] * w[idx, 1, j] * w[idx, 2, k]
        np.add.at(out[0], cell, np.rint(wt * FIELD_OBS_DENSITY_FIX).astype(np.int64) if quantise else wt)
        for b in range(channels - 1):
            m = wt * v[idx, b]
            np.add.at(out[1 + b], cell, np.rint(m * FIELD_OBS_MOMENTUM_FIX).astype(np.int64) if quantise else m)
    if quantise:
        out = np.concatenate([out[:1].astype(np.float64) / FIELD_OBS_DENSITY_FIX, out[1:].astype(np.float64) / FIELD_OBS_MOMENTUM_FIX])
    return out.reshape((channels,) + n)


def field_obs_grad_of_points(x, v, spec, G, terms=False):
    """the adjoint of field_obs_of_points for a cotangent G [channels, n0, n1, n2]: (gx, gv) [M, 3] fp64, summed over the in-field stencil
    cells in the engine's order i, j, k:  gx_a = sum_c (G_0[c] + sum_b G_{1+b}[c] v_b) d w_pc / d x_a,  gv_b = sum_c G_{1+b}[c] w_pc (zero
    with one channel).  Guarded points have zero rows.  terms=True: also (ax, av), the sums of the absolute values of the terms."""
    G = np.asarray(G, np.float64)
    channels = G.shape[0]
    assert channels in (1, 4), 'channels must be 1 or 4'
    G = G.reshape(channels, -1)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    ok, base, w, dw = field_obs_ok(x, v, spec)
    gx, gv = np.zeros((len(ok), 3), np.float64), np.zeros((len(ok), 3), np.float64)
    ax, av = np.zeros_like(gx), np.zeros_like(gv)
    for (i, j, k), idx, cell in _stencil_cells(spec, ok, base):
        wt = w[idx, 0, i] * w[idx, 1, j] * w[idx, 2, k]
        coef = G[0, cell].copy()
        acoef = np.abs(coef)
        for b in range(channels - 1):
            gb = G[1 + b, cell]
            coef += gb * v[idx, b]
            acoef += np.abs(gb * v[idx, b])
            gv[idx, b] += gb * wt
            av[idx, b] += np.abs(gb * wt)
        d = (dw[idx, 0, i] * w[idx, 1, j] * w[idx, 2, k], w[idx, 0, i] * dw[idx, 1, j] * w[idx, 2, k], w[idx, 0, i] * w[idx, 1, j] * dw[idx, 2, k])
        for a in range(3):
            gx[idx, a] += coef * d[a]
            ax[idx, a] += acoef * np.abs(d[a])
    return (gx, gv, ax, av) if terms else (gx, gv)


def cloud_point_ok(x, mask):
    """[M] bool: may a point be a query or a candidate under the axis mask?  Not with a non-finite word, nor with
    |x_a| > FE_CLOUD_COORD_MAX on an axis of the mask."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    ok = np.isfinite(x).all(axis=1)
    for a in _axes(mask):
        with np.errstate(invalid='ignore'):
            ok &= np.abs(x[:, a]) <= _capi.FE_CLOUD_COORD_MAX
    return ok


def nearest_bruteforce(q, c, mask, chunk=256):
    """for every row of q [Q, 3] the nearest row of c [M, 3] on the axes of `mask`, by all pairs in fp64 (the engine's bits when the
    coordinates are fp32 words, in a float32 or a float64 array):
    d_a = (double)q_a - (double)c_a (0 on an axis outside the mask), d2 = (d_x d_x + d_y d_y) + d_z d_z, the smallest d2 wins and among
    equal d2 the lowest row of c.  Rows that fail cloud_point_ok are skipped on both sides: such a row of q gets (-1, 0), such a row of c
    is no candidate; without a candidate every row of q gets (-1, 0).  Returns (nn [Q] int64, d2 [Q] float64)."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    c = np.asarray(c, np.float64).reshape(-1, 3)
    nn, d2 = np.full((len(q),), -1, np.int64), np.zeros((len(q),), np.float64)
    qi, ci = np.nonzero(cloud_point_ok(q, mask))[0], np.nonzero(cloud_point_ok(c, mask))[0]
    if len(qi) == 0 or len(ci) == 0:
        return nn, d2
    m = np.array([float((mask >> a) & 1) for a in range(3)])
    cc = c[ci] * m                                           # (a masked axis: 0 - 0)
    for lo in range(0, len(qi), chunk):
        rows = qi[lo:lo + chunk]
        d = (q[rows] * m)[:, None, :] - cc[None, :, :]
        dd = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        j = dd.argmin(axis=1)                                # (the first of equal minima: the lowest row)
        nn[rows] = ci[j]
        d2[rows] = dd[np.arange(len(rows)), j]
    return nn, d2


def eval_terms_numpy(terms, x, used, mat, ref=None, want_grad=False, fields=None, targets=None, clouds=None, cover_quantise=True):
    """values [n_terms] (fp64) of the program on one frame and, with want_grad, d sum_t value_t / d x as [N, 3] fp64 (else None).
    x [N, 3], used [N], mat [N] by particle id; ref [N, 3] for L1_REF; fields / targets: the DensityField and the target array of every
    field id a DENSITY_SQ term names (dicts or sequences).  |d|' = sign(d), 0 at d == 0; the gradient of a particle is summed over the
    terms in their order.  clouds: the points [M, 3] of every cloud id a NEAREST_SQ / COVER_SQ term names (dict or sequence); the COVER
    gradient is summed in the engine's fixed point (np.rint(d 2^40) in int64) unless cover_quantise is False."""
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
        elif T.kind == DENSITY_SQ:
            assert fields is not None and targets is not None, 'DENSITY_SQ needs fields and targets'
            spec = fields[T.field]
            r = density_of_points(x[ia], spec) - np.asarray(targets[T.field], np.float64).reshape(spec.shape)
            values[t] = T.weight * float((r * r).sum())
            if want_grad:
                grad[ia] += T.weight * density_grad_of_points(x[ia], spec, 2.0 * r)
        elif T.kind in (NEAREST_SQ, COVER_SQ):
            assert clouds is not None, 'NEAREST_SQ / COVER_SQ need clouds'
            tc = np.asarray(clouds[T.cloud], np.float64).reshape(-1, 3)
            axes = _axes(T.axis_mask)
            if T.kind == NEAREST_SQ:                         # queries: the selected particles; nn: rows of the cloud
                nn, d2 = nearest_bruteforce(x[ia], tc, T.axis_mask)
                values[t] = T.weight * float(d2.sum())
                if want_grad:
                    hit = nn >= 0
                    for a in axes:
                        grad[ia[hit], a] += (2.0 * (x[ia[hit], a] - tc[nn[hit], a])) * T.weight
            else:                                            # queries: the cloud points; nn: rows of x[ia], in pid order
                nn, d2 = nearest_bruteforce(tc, x[ia], T.axis_mask)
                values[t] = T.weight * float(d2.sum())
                if want_grad and (nn >= 0).any():
                    p = ia[nn[nn >= 0]]
                    for a in axes:
                        d = x[p, a] - tc[nn >= 0, a]
                        if cover_quantise:
                            words = np.zeros((len(x),), np.int64)
                            np.add.at(words, p, np.rint(d * COVER_FIX).astype(np.int64))
                            tot = words.astype(np.float64) / COVER_FIX
                        else:
                            tot = np.zeros((len(x),), np.float64)
                            np.add.at(tot, p, d)
                        touched = np.zeros((len(x),), bool)
                        touched[p] = True
                        grad[touched, a] += (2.0 * tot[touched]) * T.weight
        else:
            raise ValueError(f'unknown term kind {T.kind}')
    return values, grad
