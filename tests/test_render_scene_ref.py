"""tests/render_scene_ref.py -- the numpy restatement the GPU scene pictures are compared with -- checked against facts that need no
renderer: an analytic sphere SDF sampled at res 24 behind a scaling and translating T.  No GPU, no engine."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import render_ref as RR  # noqa: E402
import render_scene_ref as RS  # noqa: E402

RES, LO, HI = 24, np.array([0.1, 0.15, 0.05]), np.array([0.9, 0.8, 0.95])
CENTRE, RADIUS = np.array([0.5, 0.45, 0.5]), 0.25
LIGHTS = dict(ambient=np.full(3, 0.1), background=np.ones(3), pos=np.array([[0.5, 1.5, 0.5], [0.5, 1.5, 1.5]]), color=np.full((2, 3), 0.5))


def sphere_volume(value=None):
    h = (HI - LO) / (RES - 1)
    g = [LO[a] + np.arange(RES) * h[a] for a in range(3)]
    X, Y, Z = np.meshgrid(*g, indexing='ij')
    vox = np.sqrt((X - CENTRE[0]) ** 2 + (Y - CENTRE[1]) ** 2 + (Z - CENTRE[2]) ** 2) - RADIUS
    if value is not None:
        vox = np.full_like(vox, value)
    T = np.eye(4)
    for a in range(3):
        T[a, a] = 1.0 / h[a]; T[a, 3] = -LO[a] / h[a]
    return RS.volume(vox, T, (200, 90, 40, 255)), h


@pytest.fixture(scope='module')
def picture():
    cam = RR.camera((97, 61), (0.4, 0.9, 2.1), (0.5, 0.45, 0.5), 30)
    V, h = sphere_volume()
    return cam, V, h, RS.render_scene(cam, LIGHTS, 7, volumes=[(3, V)])


def _analytic(cam):
    """per pixel: the ray-sphere root in t (nan: none), the direction, and the distance of the ray from the centre"""
    d, _, _, _ = RS.ray(cam, dict(p=None, T=np.eye(4, dtype=np.float32)[:3].reshape(12)))
    oc = cam['pos'] - CENTRE
    A = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    B = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2]
    C = float(oc @ oc) - RADIUS * RADIUS
    disc = B * B - A * C
    with np.errstate(invalid='ignore'):
        root = (-B - np.sqrt(disc)) / A
    miss_dist = np.sqrt(np.maximum(float(oc @ oc) - B * B / A, 0.0))
    return root, np.sqrt(A), miss_dist


def test_silhouette_is_the_analytic_disc_up_to_one_voxel(picture):
    cam, V, h, ref = picture
    root, _, dist = _analytic(cam)
    inside, voxel = dist < RADIUS, float(h.max())
    sure = np.abs(dist - RADIUS) > voxel
    assert sure.sum() > 0.8 * sure.size and (inside & sure).sum() > 100
    assert np.array_equal(ref['covered'][sure], inside[sure])
    assert set(np.unique(ref['id'])) == {-1, RS.vol_id0(7) + 3}
    assert np.all(np.isinf(ref['depth'][~ref['covered']])) and np.all(ref['rgb'][~ref['covered']] == 255)


def test_hit_depth_is_within_one_voxel_along_the_ray(picture):
    cam, V, h, ref = picture
    root, dlen, dist = _analytic(cam)
    m = ref['covered'] & (dist < RADIUS)
    # one voxel length in world units along the ray, in units of t (the ray's direction has length dlen)
    err = np.abs(ref['depth'][m].astype(np.float64) - root[m]) * dlen[m]
    assert err.max() <= float(h.max()), err.max()
    assert ref['fragile'].sum() <= 0.005 * ref['covered'].sum()
    # lit from above: the upper half of the ball is brighter than the lower
    jj = np.nonzero(m.any(axis=1))[0]
    assert ref['rgb'][jj[2]][m[jj[2]]].mean() > ref['rgb'][jj[-3]][m[jj[-3]]].mean()


def test_a_ray_that_misses_the_box_leaves_the_background():
    cam = RR.camera((31, 17), (0.4, 0.9, 2.1), (0.4, 2.0, 4.0), 30)           # looking away
    V, _ = sphere_volume()
    ref = RS.render_scene(cam, LIGHTS, 0, volumes=[(0, V)])
    assert not ref['covered'].any() and np.all(ref['id'] == -1) and np.all(ref['rgb'] == 255)


def test_a_camera_inside_the_solid_hits_at_t0():
    cam = RR.camera((31, 17), (0.5, 0.45, 0.5), (0.5, 0.45, 0.0), 30, near=0.02)    # at the centre of the box, solid everywhere
    V, _ = sphere_volume(value=-1.0)
    ref = RS.render_scene(cam, LIGHTS, 0, volumes=[(5, V)])
    assert ref['covered'].all() and np.all(ref['id'] == RS.vol_id0(0) + 5)
    assert np.all(ref['depth'] == np.float32(0.02))


def test_spheres_and_volumes_share_the_depth_order(picture):
    cam, V, h, _ = picture
    x = np.array([[0.5, 0.45, 1.2], [0.5, 0.45, -0.2]], np.float32)           # one in front of the ball, one behind it
    ref = RS.render_scene(cam, LIGHTS, 2, x=x, ids=[0, 1], radius=0.05, rgba=[[10, 200, 10, 255]] * 2, volumes=[(0, V)])
    assert (ref['id'] == 0).sum() > 10 and (ref['id'] == 1).sum() == 0 and (ref['id'] == RS.vol_id0(2)).sum() > 100
    only = RR.render(cam, LIGHTS, x[:1], [0], 0.05, [[10, 200, 10, 255]])
    m = ref['id'] == 0
    assert np.array_equal(only['id'][m], ref['id'][m]) and np.array_equal(only['depth'][m], ref['depth'][m]) and np.array_equal(only['rgb'][m], ref['rgb'][m])
