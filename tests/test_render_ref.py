"""Invariants of the numpy restatement of the renderer's contract (tests/render_ref.py), which the GPU tests compare against: the nearer of
two overlapping spheres wins, of two identical spheres the lower id, the order of the input does not matter, nothing behind the camera is
drawn, a sub-pixel sphere keeps its centre pixel.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import render_ref as RR  # noqa: E402

CAM = RR.camera((64, 48), (0.5, 0.5, 3.0), (0.5, 0.5, 0.5), 40.0, max_radius_px=32.0)
LIGHTS = dict(ambient=np.full(3, 0.1), background=np.ones(3), pos=np.array([[0.5, 1.5, 0.5], [0.5, 1.5, 1.5]]), color=np.full((2, 3), 0.5))
RED, GREEN = (255, 0, 0, 255), (0, 255, 0, 255)


def _draw(x, ids, radius, rgba):
    return RR.render(CAM, LIGHTS, np.asarray(x, np.float32), ids, radius, np.asarray(rgba, np.uint8))


def test_the_nearer_of_two_overlapping_spheres_wins():
    out = _draw([[0.5, 0.5, 1.0], [0.58, 0.5, 1.5]], [0, 1], 0.1, [RED, GREEN])
    centre = out['id'][24, 32]
    assert centre == 1 and out['id2'][24, 32] == 0 and out['depth'][24, 32] < out['depth2'][24, 32]
    assert (out['id'] == 0).any() and (out['id'] == 1).any()                     # the farther one shows beside the nearer
    g = out['rgb'][out['id'] == 1]
    assert g[:, 1].max() > 60 and np.all(g[:, 0] == 0) and np.all(g[:, 2] == 0)
    assert np.all(out['rgb'][out['id'] == -1] == 255) and np.all(np.isinf(out['depth'][out['id'] == -1]))
    # swapping the ids does not change who is nearer
    assert np.array_equal(_draw([[0.5, 0.5, 1.0], [0.58, 0.5, 1.5]], [1, 0], 0.1, [RED, GREEN])['depth'], out['depth'])


def test_of_two_identical_spheres_the_lower_id_wins():
    out = _draw([[0.5, 0.5, 1.0], [0.5, 0.5, 1.0]], [7, 3], 0.1, [RED, GREEN])
    cov = out['covered']
    assert cov.sum() > 20 and np.all(out['id'][cov] == 3) and np.all(out['id2'][cov] == 7)
    assert np.array_equal(out['depth'][cov], out['depth2'][cov]) and not out['fragile'][cov].any()      # twins: an exact tie, decided by the ids
    near = _draw([[0.5, 0.5, 1.0], [0.5, 0.5, np.nextafter(np.float32(1.0), np.float32(2.0))]], [7, 3], 0.1, [RED, GREEN])
    assert near['fragile'][cov].any()                                                 # a last-bit difference in depth is fragile


def test_input_order_does_not_matter():
    rng = np.random.RandomState(1)
    x = rng.uniform(0.1, 0.9, (300, 3)).astype(np.float32)
    ids = np.arange(300)
    rgba = rng.randint(0, 256, (300, 4)).astype(np.uint8)
    a = _draw(x, ids, 0.04, rgba)
    p = rng.permutation(300)
    b = _draw(x[p], ids[p], 0.04, rgba[p])
    for k in ('rgb', 'depth', 'id', 'depth2', 'id2', 'fragile'):
        assert np.array_equal(a[k], b[k]), k
    assert a["covered"].sum() > 300 and not a['fragile'].all()


def test_nothing_behind_the_camera_or_non_finite_is_drawn():
    nan, inf = float('nan'), float('inf')
    out = _draw([[0.5, 0.5, 3.5], [0.5, 0.5, 2.95], [nan, 0.5, 1.0], [0.5, inf, 1.0], [0.5, 0.5, -inf]], np.arange(5), 0.1, [RED] * 5)
    assert not out['covered'].any() and np.all(out['id'] == -1) and np.all(out['rgb'] == 255)
    assert RR.project(CAM, [0.5, 0.5, 2.95], 0.1) is None and RR.project(CAM, [0.5, 0.5, 2.85], 0.1) is not None      # near + R = 0.11


def test_a_sub_pixel_sphere_keeps_its_centre_pixel_and_the_radius_is_clamped():
    out = _draw([[0.8, 0.7, -30.0]], [5], 0.001, [RED])
    assert out['covered'].sum() == 1 and out['n_subpixel'] == 1
    sp = RR.project(CAM, [0.8, 0.7, -30.0], 0.001)
    assert out['id'][sp['cj'], sp['ci']] == 5
    cam = dict(CAM, max_radius_px=4.0)
    sp = RR.project(cam, [0.5, 0.5, 2.5], 0.1)
    assert sp['clamped'] and sp['rp'] == 4.0 and sp['i1'] - sp['i0'] + 1 <= 10
