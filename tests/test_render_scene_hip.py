"""The scene in the renderer's picture on the GPU (include/fluidengine_ext.h: fe_render_set_volume, fe_render_set_scene,
fe_render_scene_frame) against the numpy restatement of its contract (tests/render_scene_ref.py): id and depth bit for bit, RGB within one
level outside the pixels the restatement calls fragile.  The smallest shapes at which the kernels can still go wrong: an image of 97 x 61
(a partial last workgroup, a width that is no multiple of the wave), a smoke grid of 16 with the slab 6 < j < 10, volumes at res 12 and
res 3, 300 particles on frame 12, behind the first sort."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import render_ref as RR  # noqa: E402
import render_scene_ref as RS  # noqa: E402
import scenarios as S  # noqa: E402
from fluidlab_amd import _capi  # noqa: E402
from fluidlab_amd.fluidengine.renderers import hip_renderer as HR  # noqa: E402

pytestmark = pytest.mark.gpu

N, RES, R = 300, (97, 61), 0.03
F = 12                                                           # a frame behind the first sort (sort interval 10)
NS = 4                                                           # substeps per step: frame 12 is the end of step 3
SMOKE_N, LO, HI = 16, 6, 10
CAM = dict(camera_pos=(0.45, 0.62, 2.2), camera_lookat=(0.5, 0.5, 0.5), fov=25, max_radius_px=8.0)
LIGHTS = [{'pos': (0.5, 1.5, 0.5), 'color': (0.5, 0.5, 0.5)}, {'pos': (0.5, 1.5, 1.5), 'color': (0.5, 0.5, 0.5)}]
AMBIENT = (0.1317, 0.1123, 0.1231)    # (not 0.1: on a pixel no light reaches, 0.1 puts every base colour ending in 5 on a rounding boundary; these put none there)
HUGE = 2 ** 31 - 1
COLD, HOT = HR.SMOKE_COLD, HR.SMOKE_HOT
SPHERE_C, SPHERE_R = np.array([0.33, 0.5, 0.5]), 0.16
COL = {'sphere': (200, 90, 40, 255), 'block': (30, 160, 90, 255), 'box': (120, 110, 230, 255), 'own': (240, 220, 30, 255)}
SLOT = {'sphere': 0, 'block': 5, 'box': 15, 'own': 9}


def _box_T(res, lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    T = np.eye(4)
    for a in range(3):
        T[a, a] = (res - 1) / (hi[a] - lo[a]); T[a, 3] = -lo[a] * T[a, a]
    return T


def _sphere_static():
    """a sphere SDF at res 12 in a box with three different voxel sizes (a non-uniform T), scaled as the stand-ins are"""
    lo, hi = (0.1, 0.2, 0.25), (0.6, 0.85, 0.8)
    g = [np.linspace(lo[a], hi[a], 12) for a in range(3)]
    X, Y, Z = np.meshgrid(*g, indexing='ij')
    vox = 0.7 * (np.sqrt((X - SPHERE_C[0]) ** 2 + (Y - SPHERE_C[1]) ** 2 + (Z - SPHERE_C[2]) ** 2) - SPHERE_R)
    return S.f32(vox), _box_T(12, lo, hi)


def _block_static():
    """res 3 (2^3 cells), solid throughout"""
    return S.f32(np.full((3, 3, 3), -1.0)), _box_T(3, (0.68, 0.15, 0.4), (0.84, 0.33, 0.62))


def _at(cam, px, py, zc):
    W, H = cam['width'], cam['height']
    return cam['pos'] + zc * (cam['fwd'] + ((px - 0.5 * W) / cam['focal']) * cam['right'] - ((py - 0.5 * H) / cam['focal']) * cam['up'])


def _q_ramp(seed, s):
    """component 0 of a smoke frame: a ramp over the grid with one NaN and one value above 1 inside the slab"""
    i, j, k = np.meshgrid(np.arange(SMOKE_N), np.arange(SMOKE_N), np.arange(SMOKE_N), indexing='ij')
    q = ((i + 2 * k + 3 * j + 5 * s + seed) % 23 + 0.3) / 23.0      # (never 0.5: that channel would sit on a rounding boundary)
    q = q.astype(np.float32)
    q[3, 8, 15] = np.nan                                          # front face of the slab (k = 15 faces the camera)
    q[9, 7, 15] = 1.75
    return q


class World:
    """one engine with everything in it, stepped to frame 12; the pieces are switched on per test"""

    def __init__(self, hiplib):
        self.cam_c = HR.make_camera(RES, CAM['camera_pos'], CAM['camera_lookat'], CAM['fov'], max_radius_px=CAM['max_radius_px'])
        self.lights_c = HR.make_lights(LIGHTS, ambient=AMBIENT)
        self.cam, self.lights = RR.camera_of(self.cam_c), RR.lights_of(self.lights_c)
        sc = S.water_block(n_grid=16, n_particles=N)
        sc.update(n_substeps=NS, horizon=4)
        self.vox = {'sphere': _sphere_static(), 'block': _block_static(), 'box': S.box_sdf_mesh(half=(0.12, 0.05, 0.08), res=12, radius=0.3)}
        sc['statics'] = [dict(voxels=self.vox[k][0], T=self.vox[k][1], friction=0.0) for k in ('sphere', 'block')]
        eng = self.eng = S.make_engine(hiplib, sc, max_substeps_local=16)
        assert eng.get_option('sort_interval') == 10
        e = self.e = eng.add_effector(type=S.FE_EFF_PLAIN, action_dim=6, action_scale_v=(1,) * 6, action_scale_p=(1,) * 6,
                                      boundary=hiplib.make_boundary(type='cube', lower=(0.1, 0.1, 0.1), upper=(0.9, 0.9, 0.9)))
        eng.eff_set_mesh(e, self.vox['box'][0], self.vox['box'][1], friction=0.5, softness=0.0)
        self.e_plain = eng.add_effector(type=S.FE_EFF_PLAIN, action_dim=6, action_scale_v=(1,) * 6, action_scale_p=(1,) * 6,
                                        boundary=hiplib.make_boundary(type='cube', lower=(0.1, 0.1, 0.1), upper=(0.9, 0.9, 0.9)))      # no mesh
        st0 = eng.eff_get_state(e, 0)
        st0[:7] = [0.7, 0.78, 0.5, 0.9238795, 0.0, 0.3826834, 0.0]
        eng.eff_set_state(e, 0, st0)
        eng.smoke_create(res=SMOKE_N, dt=0.03, solver_iters=2, q_dim=1, max_steps_local=3, lower_y=LO, higher_y=HI)
        for s in range(3):                                        # turned and moved: the pose of frame 12 is not the pose of frame 0
            eng.eff_set_action(e, s, s, NS, S.f32([0.004, -0.003, 0.002, 0.05, 0.08, -0.06]))
            eng.step(s * NS, s * NS, NS, 1)
        self.pose = {f: eng.eff_get_state(e, f)[:7].copy() for f in (0, F)}
        assert np.abs(self.pose[F][:3] - self.pose[0][:3]).max() > 1e-3 and np.abs(self.pose[F][3:] - self.pose[0][3:]).max() > 1e-3
        assert abs(self.pose[F][3]) < 0.9999
        self.q = {s: _q_ramp(1, s) for s in (1, 2)}
        for s, q in self.q.items():
            eng.smoke_set_frame(s, q=q[..., None])
        eng.render_setup(self.cam_c, self.lights_c)
        rng = np.random.RandomState(4)
        self.rgba = rng.randint(30, 256, (N, 4)).astype(np.uint8)
        self.rgba[:, 3] = 255
        eng.render_set_colors(self.rgba, R)
        self.plain_before = None

    def volumes(self, f, names=('sphere', 'block', 'box')):
        out = []
        for k in names:
            pose = dict(pos=self.pose[f][:3], quat=self.pose[f][3:7]) if k == 'box' else {}
            out.append((SLOT[k], RS.volume(self.vox[k][0], self.vox[k][1], COL[k], **pose)))
        return out

    def set_volumes(self, on=True):
        eng = self.eng
        for c in range(_capi.FE_RENDER_MAX_VOLUMES):
            eng.render_set_volume(c)
        if on:
            eng.render_set_volume(SLOT['sphere'], _capi.FE_RENDER_VOL_STATIC, 0, COL['sphere'])
            eng.render_set_volume(SLOT['block'], _capi.FE_RENDER_VOL_STATIC, 1, COL['block'])
            eng.render_set_volume(SLOT['box'], _capi.FE_RENDER_VOL_EFFECTOR, self.e, COL['box'])

    def scene(self, smoke):
        sc = _capi.FeRenderScene()
        sc.march_step, sc.bisect_iters = 0.5, 10
        if smoke:
            sc.draw_smoke, sc.lo, sc.hi, sc.smoke_radius = 1, LO, HI, 1.0 / SMOKE_N
            sc.cold[:], sc.hot[:] = COLD, HOT
        return sc

    def smoke_ref(self, s):
        return dict(n=SMOKE_N, lo=LO, hi=HI, q=self.q[s], radius=1.0 / SMOKE_N, cold=COLD, hot=HOT)

    def particles(self, f):
        st = S.get_state(self.eng, f)
        d = st['used'] != 0
        return dict(x=st['x'][d], ids=np.arange(N)[d], radius=R, rgba=self.rgba[d])

    def hide_particles(self, f):
        self.eng.set_frame(f, x=S.f32(np.full((N, 3), -100.0)), used=np.zeros(N, np.int32))

    def draw(self, f, s=0):
        self.eng.render_scene_frame(f, s)
        return self.eng.render_get(True, True, True)

    def draw_plain(self, f):
        self.eng.render_frame(f)
        return self.eng.render_get(True, True, True)


@pytest.fixture(scope='module')
def world(hiplib):
    w = World(hiplib)
    w.plain_before = {f: w.draw_plain(f) for f in (0, F)}         # before any scene call
    yield w
    w.eng.close()


def _same(a, b):
    return all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(a, b))


def _check(ref, pic, min_covered, max_fragile=0.005):
    n_cov, n_fr = int(ref['covered'].sum()), int(ref['fragile'].sum())
    print(f'covered {n_cov} fragile {n_fr}')
    assert n_cov >= min_covered and n_fr <= max_fragile * n_cov    # (a condition on the scene, from the restatement alone)
    rgba, depth, ids = pic
    bad = RS.compare(ref, rgba, depth, ids, max_fragile)
    assert not bad, bad
    assert np.all(rgba[..., 3] == 255) and np.all(np.isinf(depth[ids < 0])) and np.all(rgba[ids < 0][:, :3] == 255)


def test_volumes_against_the_restatement(world):
    w = world
    w.set_volumes(True)
    w.eng.render_set_scene(w.scene(False))
    keep = {f: S.get_state(w.eng, f) for f in (0, F)}
    for f in (0, F):
        w.hide_particles(f)
    try:
        v0 = RS.vol_id0(N)
        pics = {}
        for f in (F, 0):
            ref = RS.render_scene(w.cam, w.lights, N, volumes=w.volumes(f))
            pics[f] = w.draw(f)
            _check(ref, pics[f], 600)
            seen = set(np.unique(ref['id']).tolist())
            assert seen == {-1, v0 + SLOT['sphere'], v0 + SLOT['block'], v0 + SLOT['box']}, seen
        # the effector is drawn where it was in each frame; the statics do not move
        box = v0 + SLOT['box']
        assert not np.array_equal(pics[0][2] == box, pics[F][2] == box)
        assert np.array_equal(pics[0][2] == v0 + SLOT['sphere'], pics[F][2] == v0 + SLOT['sphere'])
        # the solid block is hit at sample 0 where the first sample falls inside it: the depth of the box's face, no bisection
        assert (pics[F][2] == v0 + SLOT['block']).sum() > 30
    finally:
        for f in (0, F):
            w.eng.set_frame(f, x=keep[f]['x'], used=keep[f]['used'])


def _tie_particle(w, ref_vol, clear):
    """a particle position whose fragment at one pixel of the sphere volume has exactly the depth bits of the volume's hit there (a pixel no
    other particle covers: `clear`)"""
    cam = w.cam
    jj, ii = np.nonzero(clear & (ref_vol['id'] == RS.vol_id0(N) + SLOT['sphere']))
    c = np.argmin((jj - jj.mean()) ** 2 + (ii - ii.mean()) ** 2)
    pj, pi = int(jj[c]), int(ii[c])
    want = ref_vol['depth'][pj, pi]
    for k in range(-600, 600):
        x = S.f32(_at(cam, pi + 0.5, pj + 0.5, float(want) + R + k * 2e-8))
        sp = RR.project(cam, x, R)
        fj, fi, cov, _, _, _, dep, _ = RR.fragments(sp)
        m = (fj == pj) & (fi == pi)
        if m.any() and cov[m][0] and dep[m][0].view(np.uint32) == want.view(np.uint32):
            return x, (pj, pi)
    raise AssertionError('no particle position gives the depth bits of the volume hit')


def test_compositing(world):
    w = world
    w.set_volumes(True)
    w.eng.render_set_scene(w.scene(False))
    ref_vol = RS.render_scene(w.cam, w.lights, N, volumes=w.volumes(F))
    keep = S.get_state(w.eng, F)
    x = S.f32(np.full((N, 3), -100.0))
    used = np.zeros(N, np.int32)
    front, behind, inside, tie = np.arange(0, 20), np.arange(20, 40), np.arange(40, 60), 60
    rng = np.random.RandomState(8)
    for i in front:
        x[i] = SPHERE_C + [rng.uniform(-0.1, 0.02), rng.uniform(-0.1, 0.1), SPHERE_R + 0.1]
    for i in behind:
        x[i] = SPHERE_C + [rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08), -SPHERE_R - 0.1]
    for i in inside:
        x[i] = SPHERE_C + rng.uniform(-0.05, 0.05, 3)
    used[:60] = 1
    others = RR.render(w.cam, w.lights, x[:60], np.arange(60), R, w.rgba[:60])
    x[tie], (tj, ti) = _tie_particle(w, ref_vol, ~others['covered'])
    used[tie] = 1
    w.eng.set_frame(F, x=x, used=used)
    edge = S.f32([_at(w.cam, 14.0 + 1.5 * n, 20.0 + n, 1.55) for n in range(12)])      # a point set across the sphere's silhouette
    w.eng.render_set_points(0, edge, (250, 200, 20, 255), 0.02)
    try:
        d = used != 0
        xs = np.concatenate([x[d], edge])
        ids = np.concatenate([np.arange(N)[d], N + np.arange(12)])
        rad = np.concatenate([np.full(d.sum(), R), np.full(12, 0.02)])
        col = np.concatenate([w.rgba[d], np.tile(np.uint8([250, 200, 20, 255]), (12, 1))])
        ref = RS.render_scene(w.cam, w.lights, N, x=xs, ids=ids, radius=rad, rgba=col, volumes=w.volumes(F))
        pic = w.draw(F)
        _check(ref, pic, 600, max_fragile=0.02)                  # (the tie is built to be fragile, with the pixels around it: ids and depths are compared there too, colours not)
        seen = set(np.unique(pic[2]).tolist())
        assert len(seen & set(front.tolist())) >= 15 and not seen & set(behind.tolist()) and not seen & set(inside.tolist())
        assert len(seen & set(range(N, N + 12))) >= 4 and RS.vol_id0(N) + SLOT['sphere'] in seen
        # equal depth bits: the particle's id is below every volume id, so it owns the pixel -- with the very depth bits of the volume's hit
        assert pic[2][tj, ti] == tie and pic[1][tj, ti].view(np.uint32) == ref_vol['depth'][tj, ti].view(np.uint32)
    finally:
        w.eng.render_set_points(0, None)
        w.eng.set_frame(F, x=keep['x'], used=keep['used'])


def test_smoke(world):
    w = world
    w.set_volumes(False)
    w.eng.render_set_scene(w.scene(True))
    keep = S.get_state(w.eng, F)
    w.hide_particles(F)
    try:
        c0 = RS.cell_id0(N)
        pics = {}
        for s in (1, 2):
            ref = RS.render_scene(w.cam, w.lights, N, smoke=w.smoke_ref(s))
            pics[s] = w.draw(F, s)
            _check(ref, pics[s], 1500)
        ids = pics[1][2]
        cells = np.unique(ids[ids >= 0]) - c0
        j = (cells // SMOKE_N) % SMOKE_N
        assert cells.min() >= 0 and cells.max() < SMOKE_N ** 3 and set(j.tolist()) == {7, 8, 9} and len(cells) >= 40
        nan_cell, hot_cell = (3 * SMOKE_N + 8) * SMOKE_N + 15, (9 * SMOKE_N + 7) * SMOKE_N + 15
        assert (ids == c0 + nan_cell).sum() > 0 and (ids == c0 + hot_cell).sum() > 0           # both are in the picture
        assert np.all(pics[1][0][ids == c0 + nan_cell][:, :3] == 0)                            # a non-finite q: black
        assert np.array_equal(pics[1][2], pics[2][2]) and np.array_equal(pics[1][1].view(np.uint32), pics[2][1].view(np.uint32))
        assert not np.array_equal(pics[1][0], pics[2][0])                                      # another q, another picture, the same ids
        try:
            for lane_pixels in (0, HUGE):
                w.eng.set_option('render_lane_pixels', lane_pixels)
                assert _same(pics[1], w.draw(F, 1)), lane_pixels
        finally:
            w.eng.set_option('render_lane_pixels', _capi.FE_RENDER_LANE_PIXELS)
    finally:
        w.eng.set_frame(F, x=keep['x'], used=keep['used'])


def test_everything_together_and_nothing(world):
    w = world
    assert _same(w.plain_before[F], w.draw_plain(F))
    w.set_volumes(True)
    w.eng.render_set_scene(w.scene(True))
    tgt = S.f32(np.random.RandomState(6).uniform(0.25, 0.75, (200, 3)) + np.array([0.0, 0.25, 0.3]))
    w.eng.render_set_points(0, tgt, (250, 200, 20, 255), 0.02)
    try:
        p = w.particles(F)
        assert len(p['ids']) == N
        xs = np.concatenate([p['x'], tgt]); ids = np.concatenate([p['ids'], N + np.arange(200)])
        rad = np.concatenate([np.full(N, R), np.full(200, 0.02)])
        col = np.concatenate([p['rgba'], np.tile(np.uint8([250, 200, 20, 255]), (200, 1))])
        ref = RS.render_scene(w.cam, w.lights, N, x=xs, ids=ids, radius=rad, rgba=col, volumes=w.volumes(F), smoke=w.smoke_ref(1))
        pic = w.draw(F, 1)
        _check(ref, pic, 2000)
        got = pic[2]
        assert (got >= RS.cell_id0(N)).sum() > 100 and ((got >= RS.vol_id0(N)) & (got < RS.cell_id0(N))).sum() > 100
        assert ((got >= 0) & (got < N)).sum() > 20 and ((got >= N) & (got < N + 200)).sum() > 20
        assert _same(pic, w.draw(F, 1))                          # two renders in a row
    finally:
        w.eng.render_set_points(0, None)
    # nothing: no scene, every slot cleared
    w.eng.render_set_scene(None)
    w.set_volumes(False)
    assert _same(w.plain_before[F], w.draw(F, 1)) and _same(w.plain_before[0], w.draw(0, 99))       # (s is ignored without smoke)
    assert _same(w.plain_before[F], w.draw_plain(F)) and _same(w.plain_before[0], w.draw_plain(0))


def test_an_own_copy_is_drawn_and_freed(world):
    w = world
    w.set_volumes(False)
    w.eng.render_set_scene(None)
    keep = S.get_state(w.eng, F)
    w.hide_particles(F)
    try:
        bytes0 = w.eng.get_stats(0)['bytes_state']
        vox, T = w.vox['sphere']
        w.eng.render_set_volume(SLOT['own'], _capi.FE_RENDER_VOL_OWN, 0, COL['own'], vox, T)
        ref = RS.render_scene(w.cam, w.lights, N, volumes=[(SLOT['own'], RS.volume(vox, T, COL['own']))])
        _check(ref, w.draw(F), 300)
        w.eng.render_set_volume(SLOT['own'], _capi.FE_RENDER_VOL_OWN, 0, COL['block'], *w.vox['block'])       # replaced: the first copy is freed
        w.eng.render_set_volume(SLOT['own'])
        assert w.eng.get_stats(0)['bytes_state'] == bytes0        # both copies are off the engine's byte count again
        assert _same(w.plain_before[0], w.draw(0))
    finally:
        w.eng.set_frame(F, x=keep['x'], used=keep['used'])


def test_errors_leave_the_previous_state(world, hiplib):
    w = world
    eng, lib, h = w.eng, w.eng.lib, w.eng.h
    w.set_volumes(True)
    eng.render_set_scene(w.scene(True))
    before = w.draw(F, 1)

    def keep(call, match):
        with pytest.raises(Exception, match=match):
            call()
        assert _same(before, w.draw(F, 1)), match

    for slot in (-1, _capi.FE_RENDER_MAX_VOLUMES):
        keep(lambda: eng.render_set_volume(slot, _capi.FE_RENDER_VOL_STATIC, 0, COL['own']), 'slot out of range')
    for i in (-1, 2):
        keep(lambda: eng.render_set_volume(SLOT['sphere'], _capi.FE_RENDER_VOL_STATIC, i, COL['own']), 'static index out of range')
    for e in (-1, 2):
        keep(lambda: eng.render_set_volume(SLOT['box'], _capi.FE_RENDER_VOL_EFFECTOR, e, COL['own']), 'effector index out of range')
    keep(lambda: eng.render_set_volume(SLOT['box'], _capi.FE_RENDER_VOL_EFFECTOR, w.e_plain, COL['own']), 'has no mesh')
    keep(lambda: eng.render_set_volume(SLOT['box'], 7, 0, COL['own']), 'unknown source')
    keep(lambda: eng.render_set_volume(SLOT['sphere'], _capi.FE_RENDER_VOL_OWN, 0, COL['own']), 'needs a FeSdfDesc and voxels')
    keep(lambda: eng._ck(lib.fe_render_set_volume(h, SLOT['sphere'], _capi.FE_RENDER_VOL_STATIC, 0, None, None, None)), 'null colour')

    def scene(**kw):
        sc = w.scene(True)
        for k, v in kw.items():
            setattr(sc, k, v)
        return sc

    keep(lambda: eng._ck(lib.fe_render_set_scene(h, C.byref(w.scene(True)), C.sizeof(_capi.FeRenderScene) - 8)), 'FeRenderScene size')
    for v in (0.0, -0.5, 1.5, float('nan'), float('inf')):
        keep(lambda: eng.render_set_scene(scene(march_step=v)), 'march_step')
    for v in (0.0, -1.0, float('nan'), float('inf')):
        keep(lambda: eng.render_set_scene(scene(smoke_radius=v)), 'smoke radius')
    for v in (-1, 33):
        keep(lambda: eng.render_set_scene(scene(bisect_iters=v)), 'bisect_iters')
    for lo, hi in ((-2, 5), (3, SMOKE_N + 1), (9, 9), (10, 4)):
        keep(lambda: eng.render_set_scene(scene(lo=lo, hi=hi)), 'outside the grid')
    for s in (-1, 4):
        keep(lambda: eng.render_scene_frame(F, s), r'outside \[0, max_steps_local\]')
    for f in (-1, 17):
        keep(lambda: eng.render_scene_frame(f, 1), 'frame index out of range')
    # no smoke field, and nothing before fe_render_setup
    fresh = S.make_engine(hiplib, S.water_block(n_grid=16, n_particles=64), max_substeps_local=4)
    for call in (lambda: fresh.render_set_volume(0), lambda: fresh.render_set_scene(w.scene(False)), lambda: fresh.render_scene_frame(0, 0)):
        with pytest.raises(Exception, match='fe_render_setup first'):
            call()
    fresh.render_setup(w.cam_c, w.lights_c)
    fresh.render_set_colors(np.zeros((64, 4), np.uint8), 0.02)
    with pytest.raises(Exception, match='without a smoke field'):
        fresh.render_set_scene(w.scene(True))
    fresh.render_set_scene(w.scene(False))
    fresh.render_scene_frame(0, 0)
    a = fresh.render_get(True, True, True)
    fresh.render_frame(0)
    assert _same(a, fresh.render_get(True, True, True))
    fresh.close()


def _smoke_words(eng, s):
    fr = eng.smoke_get_frame(s, ('v', 'q'))
    return {k: np.ascontiguousarray(v, np.float32).view(np.uint32) for k, v in fr.items()}


def _small_picture(te):
    """the environment's own camera at 160 x 160 (the restatement is numpy), and the ambient light of this file's scene instead of 0.1"""
    r = te.renderer
    scale = 160 / r.res[1]
    r.res = (160, 160)
    r.camera.width, r.camera.height = r.res
    r.camera.focal = r.camera.focal * scale
    r.lights.ambient[:] = AMBIENT
    te.simulator.engine.render_setup(r.camera, r.lights)


def _circulation(render, **kw):
    from fluidlab_amd.envs import make
    env = make('Circulation-v0', seed=0, loss=False, renderer_type='HIP', res=32, horizon=6, solver_iters=10, max_substeps_local=None, **kw)
    te = env.taichi_env
    _small_picture(te)
    return env, te


def _circulation_rollout(render):
    env, te = _circulation(render)
    eng = te.simulator.engine
    eng.profile_enable(True)
    if render:
        env.enable_scene_render()
    pol = env.demo_policy()
    te.apply_agent_action_p(pol.get_actions_p())
    n_seen = []
    for i in range(6):
        te.step(pol.get_action_v(i))
        if render:
            ids = te.render_buffers()[2]
            n_seen.append(int((ids >= 0).sum()))
    smoke = [_smoke_words(eng, s) for s in range(7)]
    n = eng.N
    xs = []
    for f in range(te.simulator.cur_substep_local + 1):
        x = np.zeros((n, 3), np.float32)
        eng.get_frame(f, x=x)
        xs.append(x.view(np.uint32))
    launches = {k: c for k, (ms, c) in eng.profile_read().items()}
    eng.close()
    return smoke, xs, launches, n_seen


def test_scene_pictures_leave_the_rollout_as_it_is():
    """v and q of every smoke frame and x of every particle frame, word for word where two plain runs agree word for word; otherwise within
    4 x what the two plain runs lie apart (relative to the field's range), as tests/test_render_hip.py bounds its rollout."""
    a, xa, la, seen = _circulation_rollout(True)
    b, xb, lb, _ = _circulation_rollout(False)
    c, xc, _, _ = _circulation_rollout(False)
    assert min(seen) > 1000
    assert la == lb and sum(lb.values()) > 0, (la, lb)
    assert all(np.array_equal(p, q) for p, q in zip(xa, xb)) and len(xa) == len(xb) > 1
    for s in range(7):
        for k in ('v', 'q'):
            if np.array_equal(b[s][k], c[s][k]):
                assert np.array_equal(a[s][k], b[s][k]), (s, k)
            else:
                fa, fb, fc = (w[s][k].view(np.float32).astype(np.float64) for w in (a, b, c))
                rng_ = max(1.0, float(np.abs(fb).max()))
                assert np.abs(fa - fb).max() / rng_ <= 4.0 * np.abs(fc - fb).max() / rng_ + 4e-6, (s, k)


def test_circulation_env_shows_the_room_and_the_smoke():
    env, te = _circulation(True)
    eng, r, sim = te.simulator.engine, te.renderer, te.simulator
    blank = te.render_buffers()
    assert np.all(blank[2] == -1) and np.all(blank[0] == 255)      # without enable_scene_render(): the blank image of today
    env.enable_scene_render()
    assert [v[1:3] for v in r.volumes] == [('static', 0)] and r.scene.draw_smoke == 1
    pol = env.demo_policy()
    te.apply_agent_action_p(pol.get_actions_p())
    first = te.render_buffers()
    for i in range(4):
        te.step(pol.get_action_v(i))
    rgb, depth, ids = te.render_buffers()
    assert np.array_equal(rgb, env.render('rgb_array'))
    sf = te.smoke_field
    st = te.statics[0]
    room = RS.volume(st.sdf_voxels_np.astype(np.float32), st.T_mesh_to_voxels_np, r.volumes[0][3])
    q = eng.smoke_get_frame(sim.cur_step_local, ('q',))['q'][..., 0]
    n = eng.N
    ref = RS.render_scene(RR.camera_of(r.camera), RR.lights_of(r.lights), n, volumes=[(0, room)],
                          smoke=dict(n=sf.n_grid, lo=sf.lower_y, hi=sf.higher_y, q=q, radius=1.0 / sf.n_grid, cold=COLD, hot=HOT))
    _check(ref, (np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=-1), depth, ids), 5000)
    assert (ids == RS.vol_id0(n)).sum() > 500 and (ids >= RS.cell_id0(n)).sum() > 500
    assert not np.array_equal(rgb, first[0])                     # the air conditioner has cooled some cells since step 0
    import torch
    dev = te.render_dev()
    assert isinstance(dev, torch.Tensor) and np.array_equal(dev.cpu().numpy()[..., :3], rgb)
    eng.close()


def test_latteart_env_shows_its_cup():
    from fluidlab_amd.envs import make
    from fluidlab_amd.fluidengine.meshes import sdf_cup
    import test_hip_env as E
    env = make('LatteArt-v0', seed=0, loss=False, renderer_type='HIP', **E.MINI)
    te = env.taichi_env
    r, sim = te.renderer, te.simulator
    _small_picture(te)
    env.reset()
    env.enable_scene_render()                                    # cup.obj is not in the asset tree and the env gives no stand-in: skipped, said so
    assert r.volumes == []
    st = te.statics[0]
    assert not st.has_dynamics
    st._sdf_arg, st.sdf_res = sdf_cup(0.45, 0.35, 0.06), 24
    env.enable_scene_render()
    assert [v[1] for v in r.volumes] == ['own']
    action = np.full(env.action_space.shape, 0.004, np.float32)
    for _ in range(3):
        te.step(action)
    rgb, depth, ids = te.render_buffers()
    n = sim.n_particles
    x = np.zeros((n, 3), np.float32); used = np.zeros((n,), np.int32)
    sim.engine.get_frame(sim.cur_substep_local, x=x, used=used)
    d = used != 0
    cup = RS.volume(st.sdf_voxels_np.astype(np.float32), st.T_mesh_to_voxels_np, r.volumes[0][3])
    ref = RS.render_scene(RR.camera_of(r.camera), RR.lights_of(r.lights), n, x=x[d], ids=np.arange(n)[d], radius=r.particle_radius,
                          rgba=HR.colors_to_bytes(te.particles['color'])[d], volumes=[(0, cup)])
    _check(ref, (np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=-1), depth, ids), 3000)
    assert (ids == RS.vol_id0(n)).sum() > 300 and ((ids >= 0) & (ids < n)).sum() > 300
    sim.engine.close()
