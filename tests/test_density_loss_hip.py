"""GPU: density fields of the HIP engine (fe_density_*, kernels k_density_scatter / k_density_resid, the gather in k_task_bwd) and the
FE_TERM_DENSITY_SQ term of the loss-term programs against the fp64 numpy restatement (term_program.density_of_points / eval_terms_numpy:
brute force, no quantisation).

Bounds.  A deposit is q = llrint(w 2^40): at most 2^-41 off per deposit, so a cell with k_c deposits is within k_c 2^-41 of the exact sum;
1e-12 D_ref on top covers the order of the fp64 sum on the reference's side and FMA contraction in the weights.  A value sum_c r_c^2
moves by at most sum_c 2 |r_c| k_c 2^-41 (first order) plus SUM_TOL = 1e-11 relative, the suite's bound for re-ordered fp64 sums.  A
gradient entry is scale w sum_c 2 r_c dw_pc: the engine rounds it to fp32 once (one ulp against the reference rounded to fp32) and the
quantisation of r moves it by at most |scale w| 2 sum_c |dw_pc| k_c 2^-41 -- which matters where the sum nearly cancels.  Positions on
multiples of 1/64 with origin 0 and cell 1/16 make every weight a dyadic rational, exact in fp64 and exact times 2^40: there the field
must be EQUAL to the reference."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402

from fluidlab_amd.fluidengine.losses import term_program as tp  # noqa: E402
from fluidlab_amd.fluidengine.losses.term_program import AXIS_ALL, AXIS_X, DENSITY_SQ, L1_CONST, DensityField, Sel, Term, density_of_points, eval_terms_numpy  # noqa: E402

pytestmark = pytest.mark.gpu
SUM_TOL = 1e-11
Q = 2.0 ** -41
N = 1500
F = 25


def _x_used(eng, f):
    x, used = np.zeros((eng.N, 3), np.float32), np.zeros((eng.N,), np.int32)
    eng.get_frame(f, x=x, used=used)
    return x, used


def _field_over(x, n, q):
    """a field of n cells whose stencils reach the particles between the quantiles q and 1 - q of x on every unprojected axis: a particle
    deposits when -1 <= u < n + 1, so the cells start one cell inside that range"""
    origin, cell = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    for a in range(3):
        if n[a] == 1:
            continue
        lo, hi = np.quantile(x[:, a].astype(np.float64), [q, 1.0 - q])
        cell[a] = float((hi - lo) / (n[a] + 2))
        origin[a] = float(lo + cell[a])
    return DensityField(tuple(origin), tuple(cell), tuple(n))


def _deposit_share(x, spec):
    """the share of the points x that deposit into at least one cell"""
    ok, base, _, _ = tp.density_stencil(x, spec)
    n = np.array(spec.n)
    hit = ok & np.all((base + 2 >= 0) & (base <= n - 1), axis=1)
    return hit.mean()


def _abs_dw_k(x, spec, K):
    """per point and axis sum_c |d w_pc / d x_a| k_c over the point's in-field stencil cells"""
    ok, base, w, dw = tp.density_stencil(x, spec)
    K = K.reshape(-1).astype(np.float64)
    out = np.zeros((len(x), 3))
    for (i, j, k), idx, cell in tp._stencil_cells(spec, ok, base):
        out[idx, 0] += np.abs(dw[idx, 0, i] * w[idx, 1, j] * w[idx, 2, k]) * K[cell]
        out[idx, 1] += np.abs(w[idx, 0, i] * dw[idx, 1, j] * w[idx, 2, k]) * K[cell]
        out[idx, 2] += np.abs(w[idx, 0, i] * w[idx, 1, j] * dw[idx, 2, k]) * K[cell]
    return out


class Case:
    """the shared frame: mixed materials, frame 25 (stored in a sorted order, some particles unused), and its download"""

    def __init__(self, hiplib):
        self.sc = S.mixed_materials(n_grid=16, n_particles=N)
        self.eng = S.make_engine(hiplib, self.sc, max_substeps_local=32)
        self.eng.step(0, 0, F, 0)
        self.x, self.used = _x_used(self.eng, F)
        self.mat = self.sc['mat']
        assert 0 < int(self.used.sum()) < N

    def field(self, n, sel, q=0.04):
        m = sel.mask(self.used, self.mat)
        spec = _field_over(self.x[m], n, q)
        share = _deposit_share(self.x[m], spec)
        print(f'field {n}: {int(m.sum())} selected particles, {share:.3f} of them deposit')
        assert 0.60 <= share <= 0.95                           # kept and dropped particles both occur
        return spec, m


@pytest.fixture(scope='module')
def case(hiplib):
    c = Case(hiplib)
    yield c
    c.eng.close()


GEOMETRIES = {'projected 8x1x8': (8, 1, 8), '12x10x9': (12, 10, 9), '24x20x19 (global road)': (24, 20, 19)}


@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_field_against_density_of_points(case, name):
    n = GEOMETRIES[name]
    sel = Sel(100, 1400, -1, True)
    spec, m = case.field(n, sel)
    eng = case.eng
    assert (np.prod(n) > 8192) == name.endswith('(global road)')
    eng.density_set_field(0, spec)
    D = eng.density_field(F, 0, sel)
    D_ref, K = density_of_points(case.x[m], spec, counts=True)
    assert D.shape == tuple(n) and D.dtype == np.float64
    err, bound = np.abs(D - D_ref), K * Q + 1e-12 * D_ref
    print(f'{name}: sum D {D.sum()!r} ref {D_ref.sum()!r}; max |err| {err.max()!r}, max err / bound {np.max(err[K > 0] / bound[K > 0])!r}; cells hit {int((K > 0).sum())} of {K.size}, max k_c {int(K.max())}')
    assert np.all(err <= bound) and D_ref.sum() > 0.3 * m.sum()
    assert np.all(D[K == 0] == 0)
    # sel=None is every used particle of the frame
    D_all = eng.density_field(F, 0)
    Dr, Kr = density_of_points(case.x[case.used != 0], spec, counts=True)
    assert np.all(np.abs(D_all - Dr) <= Kr * Q + 1e-12 * Dr) and D_all.sum() > D.sum()
    eng.density_set_field(0, None)


@pytest.mark.parametrize('lds', [-1, 0, 1])
def test_exact_on_dyadic_positions(hiplib, lds):
    sc = S.water_block(n_grid=16, n_particles=N)
    eng = S.make_engine(hiplib, sc, max_substeps_local=32, options={'density_lds': lds})
    assert eng.get_option('density_lds') == lds
    eng.step(0, 0, F, 0)
    rng = np.random.RandomState(6)
    x = (rng.randint(0, 64, (N, 3)) / 64.0).astype(np.float32)      # t in {0.5, 0.75, 1, 1.25}: on the stencil switch points too
    used = np.ones(N, np.int32)
    used[rng.choice(700, 90, replace=False)] = 0
    eng.set_frame(F, x=x, used=used)
    for n, cell in (((16, 16, 16), (1 / 16, 1 / 16, 1 / 16)), ((16, 1, 16), (1 / 16, 1.0, 1 / 16))):
        spec = DensityField((0.0, 0.0, 0.0), cell, n)
        eng.density_set_field(1, spec)
        D = eng.density_field(F, 1)
        D_ref = density_of_points(x[used != 0], spec)
        print(f'density_lds {lds} field {n}: sum {D.sum()!r} ref {D_ref.sum()!r}, cells that differ {int((D != D_ref).sum())}')
        assert np.array_equal(D, D_ref) and D.sum() > 1000
        assert np.array_equal(D * 2.0 ** 40, np.round(D * 2.0 ** 40))
    eng.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _programme(case):
    """two density terms on two fields and sub-ranges with a separable term between them: a gradient delivered in the wrong particle order,
    or a term skipped in the sum, cannot pass"""
    selA, selB = Sel(100, 1400, -1, True), Sel(0, 900, S.WATER, True)
    specA, mA = case.field((8, 1, 8), selA, q=0.05)
    specB, mB = case.field((12, 10, 9), selB)
    rng = np.random.RandomState(11)
    tA = density_of_points(case.x[mA], specA) * rng.uniform(0.3, 1.7, specA.shape)
    tB = rng.uniform(0.0, 3.0, specB.shape)
    terms = [Term(DENSITY_SQ, AXIS_ALL, selA, weight=0.7, field=0),
             Term(L1_CONST, AXIS_X, Sel(200, 1200, -1, True), c=(0.45, 0.0, 0.0), weight=1.3),
             Term(DENSITY_SQ, AXIS_ALL, selB, weight=-0.3, field=1)]
    return terms, {0: specA, 1: specB}, {0: tA, 1: tB}, {0: mA, 1: mB}


def _set(eng, fields, targets):
    for k in fields:
        eng.density_set_field(k, fields[k])
        eng.density_set_target(k, targets[k])


def _value_bounds(case, terms, fields, targets, masks):
    out = []
    for T in terms:
        if T.kind != DENSITY_SQ:
            out.append(0.0)
            continue
        D, K = density_of_points(case.x[masks[T.field]], fields[T.field], counts=True)
        out.append(abs(T.weight) * float((2.0 * np.abs(D - targets[T.field]) * K * Q).sum()))
    return np.array(out)


def _grad_bound(x, used, mat, terms, fields, scale):
    """per particle and axis: the propagated quantisation |scale w| 2 sum_c |dw_pc| k_c 2^-41, summed over the density terms"""
    b = np.zeros((len(x), 3))
    for T in terms:
        if T.kind != DENSITY_SQ:
            continue
        m = T.a.mask(used, mat)
        _, K = density_of_points(x[m], fields[T.field], counts=True)
        b[m] += abs(scale * T.weight) * 2.0 * _abs_dw_k(x[m], fields[T.field], K) * Q
    return b


def test_value_and_gradient(case):
    eng = case.eng
    terms, fields, targets, masks = _programme(case)
    _set(eng, fields, targets)
    eng.task_loss_alloc(2)
    eng.task_loss_set_terms(terms)
    eng.task_loss_clear()
    eng.task_loss_step(1, F)
    kw = dict(fields=fields, targets=targets)
    vals, g = eval_terms_numpy(terms, case.x, case.used, case.mat, None, True, **kw)
    sl, tl = eng.task_loss_get(2, terms=True)
    vb = _value_bounds(case, terms, fields, targets, masks)
    for t in range(3):
        bound = vb[t] + SUM_TOL * abs(vals[t])
        print(f'term {t}: got {tl[t, 1]!r} want {vals[t]!r} err {abs(tl[t, 1] - vals[t])!r} bound {bound!r}')
        assert abs(tl[t, 1] - vals[t]) <= bound and vals[t] != 0
    assert abs(sl[1] - vals.sum()) <= vb.sum() + SUM_TOL * np.abs(vals).sum() and sl[0] == 0
    assert vals[0] > 0 > vals[2]
    scale = 0.37
    eng.reset_grad()
    eng.task_loss_step_grad(1, F, scale)
    got = eng.get_grad(F)[0]
    want32 = (scale * g).astype(np.float32)
    err = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    bound = np.spacing(np.abs(want32)).astype(np.float64) + _grad_bound(case.x, case.used, case.mat, terms, fields, scale)
    sel_any = masks[0] | masks[1]
    nz = np.any(want32[sel_any] != 0, axis=1)
    print(f'gradient: max err / bound {np.max(err / bound)!r} over all {err.size} entries; {int(nz.sum())} of {int(sel_any.sum())} selected used particles have a gradient; max |g| {np.abs(want32).max()!r}')
    assert np.all(err <= bound)                               # every particle, none left out
    assert nz.sum() >= 0.5 * sel_any.sum()
    none = ~(sel_any | terms[1].a.mask(case.used, case.mat))
    assert none.sum() > 0 and np.all(got[none] == 0)
    eng.task_loss_set_terms(None)
    for k in fields:
        eng.density_set_field(k, None)


def test_roads_and_repeatability(case, hiplib):
    eng = case.eng
    terms, fields, targets, masks = _programme(case)
    _set(eng, fields, targets)
    eng.task_loss_alloc(2)
    eng.task_loss_set_terms(terms)

    def frame_words(f):                                       # (no F: this download does not expand a compact one)
        x, v, C_, u = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32), np.zeros((N, 3, 3), np.float32), np.zeros(N, np.int32)
        eng.get_frame(f, x, v, C_, None, u)
        return [_bits(a) for a in (x, v, C_)] + [u]

    before = (frame_words(F), frame_words(F - 5), eng.get_work_stats(F), eng.get_options(), eng.get_option('task_pair_chunk'))
    out = {}
    for lds in (0, 1, 0, 1):
        eng.set_option('density_lds', lds)
        eng.task_loss_clear()
        eng.task_loss_step(0, F)
        value = eng.task_loss_get(2, terms=True)
        eng.reset_grad()
        eng.task_loss_step_grad(0, F, 0.37)
        res = (eng.density_field(F, 0, terms[0].a), eng.density_field(F, 1, terms[2].a), value[0], value[1], eng.get_grad(F)[0])
        if lds in out:                                        # two evaluations on one road: the same bits
            for p, q in zip(out[lds], res):
                assert np.array_equal(_bits(p), _bits(q))
        out[lds] = res
    for p, q in zip(out[0], out[1]):                          # the two roads: the same words, hence the same values and adjoints
        assert np.array_equal(_bits(p), _bits(q))
    assert out[0][0].sum() > 0 and out[0][1].sum() > 0 and out[0][2][0] != 0 and np.abs(out[0][4]).max() > 0
    eng.set_option('density_lds', -1)
    eng.task_loss_clear()
    eng.task_loss_step(0, F)
    eng.density_field(F, 0)
    after = (frame_words(F), frame_words(F - 5), eng.get_work_stats(F), eng.get_options(), eng.get_option('task_pair_chunk'))
    for b, a in zip(before[:2], after[:2]):
        for p, q in zip(b, a):
            assert np.array_equal(p, q)
    assert before[2:] == after[2:] and eng.get_option('density_lds') == -1
    with pytest.raises(Exception, match='density_lds must be'):
        eng.set_option('density_lds', 2)
    eng.task_loss_set_terms(None)
    for k in fields:
        eng.density_set_field(k, None)


def test_adjoint_in_another_order_and_refusal(hiplib):
    sc = S.water_block(n_grid=16, n_particles=N, seed=3)
    sc['used'] = (np.random.RandomState(8).rand(N) > 0.1).astype(np.int32)
    cot = S.random_cotangent(N, seed=2)
    sel = Sel(100, 1300, -1, True)
    m = sel.mask(sc['used'], sc['mat'])
    spec = _field_over(sc['x'][m], (7, 6, 5), 0.04)
    share = _deposit_share(sc['x'][m], spec)
    assert 0.60 <= share <= 0.95
    target = np.random.RandomState(4).uniform(0.0, 30.0, spec.shape)
    terms = [Term(DENSITY_SQ, AXIS_ALL, sel, weight=0.01, field=1), Term(L1_CONST, AXIS_X, Sel(0, 400), c=(0.5, 0, 0), weight=0.2)]
    eng = S.make_engine(hiplib, sc, max_substeps_local=32, options={'sort_interval': 10, 'fuse_bwd': 1})
    eng.density_set_field(1, spec)
    eng.density_set_target(1, target)
    eng.task_loss_alloc(1)
    eng.task_loss_set_terms(terms)
    eng.step(0, 0, F, 0)
    eng.reset_grad()
    eng.add_grad(F, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad(0, 0, F, 0)                                 # back to frame 0: its adjoint is left in the order the next call's first substep works in
    g0 = eng.get_grad(0)[0]
    assert np.abs(g0).max() > 0
    eng.task_loss_step_grad(0, 0, 0.37)
    g1 = eng.get_grad(0)[0]
    x, used = _x_used(eng, 0)
    _, g = eval_terms_numpy(terms, x, used, sc['mat'], None, True, fields={1: spec}, targets={1: target})
    add32 = (0.37 * g).astype(np.float32)
    want = g0.astype(np.float64) + add32.astype(np.float64)   # one fp32 addition of the once-rounded gradient
    err = np.abs(g1.astype(np.float64) - want)
    bound = np.spacing(np.maximum(np.abs(g1), np.abs(g0))).astype(np.float64) + np.spacing(np.abs(add32)).astype(np.float64) + _grad_bound(x, used, sc['mat'], terms, {1: spec}, 0.37)
    print(f'adjoint in another order: max err / bound {np.max(err / bound)!r}; entries changed {int((g1 != g0).sum())} of {int((g != 0).sum())} with a gradient')
    assert np.all(err <= bound) and (g1 != g0).sum() > 0.5 * (g != 0).sum() and (g[400:] != 0).sum() > 500
    untouched = np.all(g == 0, axis=1)
    assert untouched.sum() >= 100 and np.array_equal(g1[untouched], g0[untouched])
    eng.close()
    # a frame whose adjoint a fused fe_step_grad passed on in registers is refused (the arrangement of test_incomplete_adjoint_slots_are_refused)
    eng = S.make_engine(hiplib, sc, options={'sort_interval': 10, 'fuse_bwd': 1})
    eng.density_set_field(1, spec)
    eng.density_set_target(1, target)
    eng.task_loss_alloc(1)
    eng.task_loss_set_terms(terms)
    eng.step(0, 0, 6, 0)
    eng.reset_grad()
    eng.add_grad(6, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad(2, 2, 4, 0)                                 # frames 5 ... 2: the slot of frame 3 is the incomplete one
    eng.task_loss_step_grad(0, 2, 1.0)                        # the call's first frame: defined
    with pytest.raises(Exception, match='registers'):
        eng.task_loss_step_grad(0, 3, 1.0)
    eng.close()


def test_errors_leave_everything_in_place(case, hiplib):
    import ctypes as C
    from fluidlab_amd import _capi
    eng = case.eng
    sel = Sel(100, 1400, -1, True)
    spec, m = case.field((8, 1, 8), sel, q=0.05)
    target = np.random.RandomState(2).uniform(0.0, 5.0, spec.shape)
    good = [Term(DENSITY_SQ, AXIS_ALL, sel, weight=0.5, field=0)]
    with pytest.raises(Exception, match='names a field that is not set'):
        eng.task_loss_set_terms(good)
    eng.density_set_field(0, spec)
    eng.task_loss_alloc(2)
    eng.task_loss_set_terms(good)
    with pytest.raises(Exception, match='has no target'):
        eng.task_loss_step(0, F)
    with pytest.raises(Exception, match='has no target'):
        eng.task_loss_step_grad(0, F, 1.0)
    eng.density_set_target(0, target)

    def still_right(tag):
        eng.task_loss_clear()
        eng.task_loss_step(0, F)
        sl, tl = eng.task_loss_get(1, terms=True)
        vals, _ = eval_terms_numpy(good, case.x, case.used, case.mat, fields={0: spec}, targets={0: target})
        D, K = density_of_points(case.x[m], spec, counts=True)
        bound = 0.5 * float((2.0 * np.abs(D - target) * K * Q).sum()) + SUM_TOL * abs(vals[0])
        print(f'{tag}: got {sl[0]!r} want {vals[0]!r} bound {bound!r}')
        assert abs(sl[0] - vals[0]) <= bound and tl[0, 0] == sl[0] and vals[0] > 0

    still_right('before the refusals')
    D = DensityField
    nan, inf = float('nan'), float('inf')
    bad_fields = [(2, spec, 'field id out of range'), (-1, spec, 'field id out of range'),
                  (0, D(spec.origin, spec.cell, (8, 0, 8)), r'n\[a\] must be >= 1'), (0, D(spec.origin, spec.cell, (-3, 1, 8)), r'n\[a\] must be >= 1'),
                  (0, D(spec.origin, spec.cell, (128, 129, 128)), 'more than FE_DENSITY_MAX_CELLS'), (0, D(spec.origin, spec.cell, (1 << 22, 1, 1)), 'more than FE_DENSITY_MAX_CELLS'),
                  (0, D(spec.origin, (0.1, 0.0, 0.1), (8, 1, 8)), 'cell must be finite and positive'), (0, D(spec.origin, (0.1, 1.0, -0.1), (8, 1, 8)), 'cell must be finite and positive'),
                  (0, D(spec.origin, (nan, 1.0, 0.1), (8, 1, 8)), 'cell must be finite and positive'), (0, D(spec.origin, (0.1, 1.0, inf), (8, 1, 8)), 'cell must be finite and positive'),
                  (0, D((0.0, nan, 0.0), spec.cell, (8, 1, 8)), 'origin must be finite')]
    for k, f, msg in bad_fields:
        with pytest.raises(Exception, match=msg):
            eng.density_set_field(k, f)
    c = spec.to_c()
    assert eng.lib.fe_density_set_field(eng.h, 0, C.byref(c), C.sizeof(_capi.FeDensitySpec) - 8) != 0
    assert b'spec_size' in eng.lib.fe_last_error(eng.h)
    for k, t, msg in ((0, np.zeros(63), 'n_cells does not match'), (0, np.zeros((8, 8, 8)), 'n_cells does not match'), (2, target, 'field id out of range'),
                      (1, target, 'field is not set')):
        with pytest.raises(Exception, match=msg):
            eng.density_set_target(k, t)
    out = np.zeros(63)
    assert eng.lib.fe_density_get(eng.h, F, 0, None, out.ctypes.data_as(C.c_void_p), C.c_longlong(63)) != 0
    assert b'n_cells does not match' in eng.lib.fe_last_error(eng.h)
    with pytest.raises(Exception, match='field is not set'):
        eng.density_field(F, 1)
    with pytest.raises(Exception, match='outside'):
        eng.density_field(F, 0, Sel(0, N + 1))
    bad_terms = [([Term(DENSITY_SQ, AXIS_ALL, sel, field=1)], 'names a field that is not set'), ([Term(DENSITY_SQ, AXIS_ALL, sel, field=2)], 'field id out of range'),
                 ([Term(DENSITY_SQ, AXIS_ALL, sel, field=-1)], 'field id out of range'), ([Term(DENSITY_SQ, AXIS_X, sel, field=0)], 'axis_mask must be 7'),
                 (good * 3, 'density terms'), ([Term(DENSITY_SQ, AXIS_ALL, Sel(0, N + 1), field=0)], 'outside'), ([Term(7, AXIS_X, Sel(0, N))], 'unknown term kind')]
    for terms, msg in bad_terms:
        with pytest.raises(Exception, match=msg):
            eng.task_loss_set_terms(terms)
    packed = good[0].to_c()
    packed.b.mat = 3
    arr = (_capi.FeLossTerm * 1)(packed)
    assert eng.lib.fe_task_loss_set_terms(eng.h, C.byref(arr), 1, C.sizeof(_capi.FeLossTerm)) != 0
    assert b'zeros in the rest of b' in eng.lib.fe_last_error(eng.h)
    still_right('after the refusals')                         # the program, field and target set before the refused calls still run
    # setting a field drops its target; removing it is noticed at the step
    eng.density_set_field(0, spec)
    with pytest.raises(Exception, match='has no target'):
        eng.task_loss_step(0, F)
    eng.density_set_field(0, None)
    with pytest.raises(Exception, match='names a field that is not set'):
        eng.task_loss_step(0, F)
    eng.task_loss_set_terms(None)
    # an engine with more than 2^23 particles is refused (created, never initialised or stepped)
    big = _capi.Engine(hiplib, n_grid=8, n_particles=(1 << 23) + 1, max_substeps_local=1, n_substeps=1, max_action_steps=1, dt=1e-4, p_vol=1e-3,
                       gravity=(0.0, -1.0, 0.0), boundary=hiplib.make_boundary())
    with pytest.raises(Exception, match=r'N > 2\^23'):
        big.density_set_field(0, spec)
    big.close()


def test_latteart_env_device_loss_against_the_host_path(hiplib):
    import test_host_env as H
    env = H._small('LatteArt-v0', None, horizon=4, horizon_action=4, loss_type='density', n_pool=300)       # None = the HIP library
    te = env.taichi_env
    loss, sim = te.loss, te.simulator
    assert sim.engine.elib.backend == 'hip-gfx950' and loss.field.shape == (64, 1, 64)
    rng = np.random.RandomState(5)
    loss.set_target_points(np.stack([rng.uniform(0.3, 0.7, 777), rng.uniform(0.5, 0.9, 777), rng.uniform(0.35, 0.65, 777)], axis=1))
    env.enable_device_loss()
    assert loss._device_loss
    pol = env.demo_policy()
    te.set_state(te.get_state()['state'], grad_enabled=True)
    te.apply_agent_action_p(pol.get_actions_p())
    host, bounds, frames = [], [], []
    mat = sim.particles_i.mat.to_numpy()
    for i in range(env.horizon):
        te.step(pol.get_action_v(i, agent=te.agent, update=True))
        s, f = sim.cur_step_global - 1, sim.cur_substep_local
        x, used = _x_used(sim.engine, f)
        m = loss.device_terms()[0].a.mask(used, mat)
        host.append(float(loss.step_value(s, f, *loss.frame(f), False)[0]))      # the interpreter on the same, still resident frame
        D, K = density_of_points(x[m], loss.field, counts=True)
        bounds.append(loss.density_weight * float((2.0 * np.abs(D - loss.target) * K * Q).sum()) + SUM_TOL * abs(host[-1]))
        frames.append((s, f, x, used, m))
    dev, host = np.array(loss.step_loss, np.float64), np.array(host)
    print(f'step_loss device {dev!r} host {host!r} err {np.abs(dev - host)!r} bound {np.array(bounds)!r}; milk in the last frame {int(frames[-1][4].sum())}')
    assert np.all(host > 0) and np.all(np.abs(dev - host) <= np.array(bounds)) and frames[-1][4].sum() > 0
    assert abs(te.get_final_loss()['loss'] - host[-1]) <= bounds[-1]
    # the image of the milk, and the x-adjoint of the last frame against the host path
    s, f, x, used, m = frames[-1]
    img = te.density_field(mat=loss.matching_mat)
    D, K = density_of_points(x[m], loss.field, counts=True)
    assert img.shape == (64, 1, 64) and np.all(np.abs(img - D) <= K * Q + 1e-12 * D)
    eng = sim.engine
    eng.reset_grad()
    loss.compute_step_loss_grad(s, f)
    g_dev = eng.get_grad(f)[0]
    loss._device_loss = False                                 # the same loss object through the host path
    try:
        eng.reset_grad()
        loss.compute_step_loss_grad(s, f)
        g_host = eng.get_grad(f)[0]
    finally:
        loss._device_loss = True
    err = np.abs(g_dev.astype(np.float64) - g_host.astype(np.float64))
    bound = np.spacing(np.abs(g_host)).astype(np.float64) + _grad_bound(x, used, mat, loss.device_terms(), {0: loss.field}, 1.0)
    print(f'x-adjoint of frame {f}: {int((g_host != 0).sum())} entries, max err / bound {np.max(err / bound)!r}')
    assert np.abs(g_host).max() > 0 and np.all(err <= bound)
