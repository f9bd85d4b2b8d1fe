"""The density term of the loss-term programs in the fp64 numpy interpreter (term_program.eval_terms_numpy with fields= / targets=,
density_of_points): its gradient against central differences, and the mass the rasteriser deposits.  No GPU, no engine.

Central differences at h = 1e-6 in fp64: the truncation error is h^2 / 6 times the third derivative of a piecewise-quadratic weight
product -- zero inside a stencil position, O(h / cell^2) only for the few points within h of a switch point -- and the rounding error
~1e-16 |value| / h ~ 1e-9.  Bound: 1e-6 relative to 1 + |g|."""
import numpy as np
import pytest

from fluidlab_amd.fluidengine.losses.term_program import (AXIS_ALL, AXIS_X, DENSITY_SQ, L1_CONST, DensityField, Sel, Term, density_of_points,
                                                          density_stencil, eval_terms_numpy)

N = 160
FIELDS = {'projected 8x1x8': DensityField((0.3, 0.0, 0.25), (0.05, 1.0, 0.06), (8, 1, 8)),
          '6x5x4': DensityField((0.3, 0.3, 0.3), (0.06, 0.07, 0.09), (6, 5, 4))}


def _points(seed=0):
    rng = np.random.RandomState(seed)
    x = rng.uniform(0.2, 0.8, (N, 3))
    used = (rng.uniform(size=N) > 0.1).astype(np.int32)
    mat = rng.randint(0, 2, N).astype(np.int32)
    return rng, x, used, mat


def _whole_stencil_inside(x, spec):
    ok, base, _, _ = density_stencil(x, spec)
    n = np.array(spec.n)
    return ok & np.all((n == 1) | ((base >= 0) & (base + 2 < n)), axis=1)


@pytest.mark.parametrize('name', list(FIELDS))
def test_gradient_against_central_differences(name):
    spec = FIELDS[name]
    rng, x, used, mat = _points()
    target = rng.uniform(0.0, 2.0, spec.shape)
    terms = [Term(DENSITY_SQ, AXIS_ALL, Sel(10, N - 10, 1, True), weight=0.7, field=1), Term(L1_CONST, AXIS_X, Sel(0, N), c=(0.5, 0, 0), weight=0.3)]
    kw = dict(fields={1: spec}, targets={1: target})
    vals, g = eval_terms_numpy(terms, x, used, mat, None, True, **kw)
    sel = terms[0].a.mask(used, mat)
    inside = _whole_stencil_inside(x, spec)
    deposits = density_of_points(x[sel], spec, counts=True)[1].sum()
    print(f'{name}: value {vals[0]!r}; selected {int(sel.sum())} of {N}, whole stencil inside {int((sel & inside).sum())}, deposits {int(deposits)}')
    assert 0 < (sel & inside).sum() < sel.sum() and vals[0] > 0           # the field covers only part of the points
    h = 1e-6
    gn = np.zeros_like(g)
    for p in range(N):
        for a in range(3):
            xp, xm = x.copy(), x.copy()
            xp[p, a] += h
            xm[p, a] -= h
            gn[p, a] = (eval_terms_numpy(terms, xp, used, mat, **kw)[0].sum() - eval_terms_numpy(terms, xm, used, mat, **kw)[0].sum()) / (2 * h)
    err = np.abs(g - gn) / (1.0 + np.abs(g))
    print(f'{name}: max |g - central difference| / (1 + |g|) = {err.max()!r}; max |g| {np.abs(g).max()!r}')
    assert err.max() <= 1e-6
    g_density = g.copy()
    g_density[:, 0] -= 0.3 * np.sign(x[:, 0] - 0.5)
    assert np.all(g_density[~sel] == 0) and np.abs(g_density[sel]).max() > 1.0      # only selected particles get a density gradient
    if spec.n[1] == 1:
        assert np.all(g_density[:, 1] == 0)                                         # none along the projected axis


@pytest.mark.parametrize('name', list(FIELDS))
def test_rasteriser_deposits_one_per_point_inside(name):
    spec = FIELDS[name]
    _, x, _, _ = _points(3)
    inside = _whole_stencil_inside(x, spec)
    assert 0 < inside.sum() < N
    D, K = density_of_points(x[inside], spec, counts=True)
    assert D.shape == spec.shape and D.dtype == np.float64
    print(f'{name}: {int(inside.sum())} points inside deposit {D.sum()!r} in {int(K.sum())} deposits')
    assert abs(D.sum() - inside.sum()) <= 1e-12 * inside.sum()
    assert K.sum() == inside.sum() * (9 if spec.n[1] == 1 else 27)
    assert density_of_points(x, spec).sum() > D.sum()                   # points at the edge deposit the part of their stencil that is inside
    # a non-finite point, or one 2^30 cells away, deposits nothing
    bad = x[:4].copy()
    bad[0, 0], bad[1, 2], bad[2, 0], bad[3, 2] = np.nan, np.inf, spec.origin[0] + spec.cell[0] * 2.0 ** 31, -1e30
    assert density_of_points(bad, spec).sum() == 0


def test_index_order_on_the_non_cubic_field():
    spec = FIELDS['6x5x4']
    centre = np.array(spec.origin) + (np.array([4, 1, 2]) + 0.5) * np.array(spec.cell)
    D = density_of_points(centre[None], spec)
    assert np.unravel_index(np.argmax(D), D.shape) == (4, 1, 2) and abs(D[4, 1, 2] - 0.75 ** 3) <= 1e-15
    assert abs(D.reshape(-1)[(4 * 5 + 1) * 4 + 2] - 0.75 ** 3) <= 1e-15


def test_term_packs_the_field_id():
    t = Term(DENSITY_SQ, AXIS_ALL, Sel(0, 5, 2, True), weight=-2.0, field=1).to_c()
    assert (t.kind, t.axis_mask, t.b.pid_lo, t.b.pid_hi, t.b.mat, t.b.require_used, t.weight) == (4, 7, 1, 0, 0, 0, -2.0)
    c = FIELDS['6x5x4'].to_c()
    assert list(c.n) == [6, 5, 4] and list(c.cell) == [0.06, 0.07, 0.09] and c.pad == 0
