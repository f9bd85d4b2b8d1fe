"""The numpy restatement of the liquid surface (tests/surface_ref.py) checked on its own: the picture does not depend on the order of the
particles, with nothing selected it is render_ref's picture, smoothing lowers the depth variance of a jittered sheet, two sheets farther
apart than `range` do not blend, the opacity is monotone in the thickness and stays inside [alpha_min, 1), and the scene the GPU tests draw
(tests/surface_cases.py) has what they need.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import render_ref as RR  # noqa: E402
import surface_cases as SC  # noqa: E402
import surface_ref as SR  # noqa: E402


@pytest.fixture(scope='module')
def scene():
    return SC.Scene()


def test_the_scene_of_the_gpu_tests_has_every_category(scene):
    figures = SC.conditions(scene)
    print(figures)


def test_picture_does_not_depend_on_the_particle_order(scene):
    P = SC.params(2, 5)
    x, ids, rad, col, d = scene.spheres()
    liquid = np.zeros(len(x), bool)
    liquid[:d.sum()] = scene.sel[d] != 0
    a = scene.ref(P)
    perm = np.random.RandomState(5).permutation(len(x))
    b = SR.render_surface(scene.cam, scene.lights, SC.N, x[perm], ids[perm], rad[perm], col[perm], liquid[perm], P)
    for k in ('rgb', 'depth', 'id', 'liq_id', 'z_raw', 'z_smooth', 'thick_words'):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_nothing_selected_is_render_ref(scene):
    x, ids, rad, col, d = scene.spheres()
    a = SR.render_surface(scene.cam, scene.lights, SC.N, x, ids, rad, col, np.zeros(len(x), bool), SC.params())
    b = RR.render(scene.cam, scene.lights, x, ids, rad, col)
    assert np.array_equal(a['rgb'], b['rgb']) and np.array_equal(a['id'], b['id']) and np.array_equal(a['depth'].view(np.uint32), b['depth'].view(np.uint32))
    assert not a['liquid'].any() and np.isinf(a['z_raw']).all() and not a['thick_words'].any()
    assert (a['fragile'] | ~b['fragile']).all()                  # (the mask holds render_ref's)


def _sheet(cam, depth, jitter, n, rng, box=(10, 60, 8, 50)):
    return np.array([SC._at(cam, rng.uniform(box[0], box[1]), rng.uniform(box[2], box[3]), depth + rng.uniform(-jitter, jitter)) for _ in range(n)], np.float32)


def test_smoothing_lowers_the_variance_of_a_jittered_sheet(scene):
    rng = np.random.RandomState(1)
    x = _sheet(scene.cam, 1.6, 0.01, 700, rng)
    n = len(x)
    P = SC.params(2, 5)
    ref = SR.render_surface(scene.cam, scene.lights, n, x, np.arange(n), SC.R, np.full((n, 4), 200, np.uint8), np.ones(n, bool), P)
    inner = np.zeros_like(ref['liquid'])
    inner[14:44, 16:54] = True                                   # away from the sheet's rim
    m = ref['liquid'] & inner
    assert m.sum() > 800
    v0, v1 = np.var(ref['z_raw'][m].astype(np.float64)), np.var(ref['z_smooth'][m].astype(np.float64))
    print(f'depth variance {v0:.3g} -> {v1:.3g}')
    assert v1 < 0.5 * v0
    one = SR.smooth(ref['z_raw'], 5, P['range'])
    assert np.var(one[m].astype(np.float64)) < v0 and np.array_equal(np.isfinite(one), ref['liquid'])      # liquid stays liquid, the rest +inf


def test_sheets_farther_apart_than_range_do_not_blend(scene):
    rng = np.random.RandomState(2)
    xa = _sheet(scene.cam, 1.6, 0.01, 300, rng, (10, 50, 8, 50))
    xb = _sheet(scene.cam, 1.6 + 3 * SC.RANGE, 0.01, 300, rng, (40, 85, 8, 50))
    x = np.concatenate([xa, xb])
    n = len(x)
    ref = SR.render_surface(scene.cam, scene.lights, n, x, np.arange(n), SC.R, np.full((n, 4), 200, np.uint8), np.ones(n, bool), SC.params(3, 8))
    liq, front = ref['liquid'], ref['liq_id'] < 300
    for m in (liq & front, liq & ~front):
        assert m.sum() > 300
        lo, hi = ref['z_raw'][m].min(), ref['z_raw'][m].max()
        assert hi - lo < SC.RANGE                                # (a sheet's own raw depths lie within `range`)
        assert (ref['z_smooth'][m] >= lo).all() and (ref['z_smooth'][m] <= hi).all()
    border = liq & front & np.roll(liq & ~front, 1, axis=1)      # pixels of one sheet beside pixels of the other exist
    assert border.sum() > 10


def test_alpha_is_monotone_and_bounded():
    for alpha_min in (0.0, 0.2, 1.0):
        for absorb in (0.0, 3.0, 1e4):
            P = SR.params(alpha_min=alpha_min, absorb=absorb)
            t = np.concatenate([[0.0], np.logspace(-9, 3, 400)])
            a = SR.alpha_of(P, t)
            assert a[0] == alpha_min and (np.diff(a) >= 0).all()
            assert (a >= alpha_min).all() and ((a < 1.0) | (alpha_min == 1.0)).all() and (a <= 1.0).all()
