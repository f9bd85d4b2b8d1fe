"""The scene of the liquid-surface tests (tests/test_surface_hip.py draws it on the GPU, tests/test_surface_ref.py checks its conditions on the
restatement alone): about 600 particles of which about 400 are liquid in two colours, an opaque point set partly in front of the liquid and
partly behind it, and one SDF volume.  A helper, not a test."""
import numpy as np

import render_ref as RR
import render_scene_ref as RS
import scenarios as S
import surface_ref as SR
from fluidlab_amd.fluidengine.renderers import hip_renderer as HR

N = 600
N_LIQUID = 400
R = 0.02
RES = (97, 61)                                                   # neither side a multiple of the 16-pixel tile, the last workgroup partial
RES_TINY = (7, 5)                                                # smaller than one tile
CAM = dict(camera_pos=(0.45, 0.62, 2.2), camera_lookat=(0.5, 0.5, 0.5), fov=40, max_radius_px=8.0)
LIGHTS = [{'pos': (0.5, 1.5, 0.5), 'color': (0.5, 0.5, 0.5)}, {'pos': (0.5, 1.5, 1.5), 'color': (0.5, 0.5, 0.5)}]
AMBIENT = (0.1317, 0.1123, 0.1231)                               # (not 0.1: see tests/test_render_scene_hip.py)
RANGE = 0.08                                                     # the two sheets lie 0.3 apart
SWEEP = [(0, 1), (1, 1), (3, 1), (0, 8), (1, 8), (3, 8)]         # (smooth_iters, smooth_radius_px)
TGT_RGBA, TGT_R = (250, 200, 20, 255), 0.02
VOL_SLOT, VOL_RGBA = 3, (200, 90, 40, 255)
Z1, Z2 = 1.6, 1.9                                                # depths of the two liquid sheets


def params(iters=2, r=5, **kw):
    return SR.params(radius_scale=1.5, smooth_iters=iters, smooth_radius_px=r, range=RANGE, absorb=25.0, alpha_min=0.2, specular=0.3, shininess_log2=4, **kw)


def params_c(P):
    from fluidlab_amd import _capi
    c = _capi.FeSurfaceParams()
    for k, v in P.items():
        setattr(c, k, v)
    return c


def _at(cam, px, py, zc):
    """the world point that projects to pixel coordinates (px, py) at depth zc"""
    W, H = cam['width'], cam['height']
    return cam['pos'] + zc * (cam['fwd'] + ((px - 0.5 * W) / cam['focal']) * cam['right'] - ((py - 0.5 * H) / cam['focal']) * cam['up'])


def sphere_volume():
    """the sphere SDF of tests/test_render_scene_hip.py: res 12 in a box with three voxel sizes, centre (0.33, 0.5, 0.5), radius 0.16"""
    lo, hi = np.array((0.1, 0.2, 0.25)), np.array((0.6, 0.85, 0.8))
    g = [np.linspace(lo[a], hi[a], 12) for a in range(3)]
    X, Y, Z = np.meshgrid(*g, indexing='ij')
    vox = 0.7 * (np.sqrt((X - 0.33) ** 2 + (Y - 0.5) ** 2 + (Z - 0.5) ** 2) - 0.16)
    T = np.eye(4)
    for a in range(3):
        T[a, a] = 11.0 / (hi[a] - lo[a]); T[a, 3] = -lo[a] * T[a, a]
    return S.f32(vox), T


class Scene:
    """positions are laid out in the pixels of the 97 x 61 camera; the 7 x 5 camera looks at the same world"""

    def __init__(self, seed=11):
        rng = np.random.RandomState(seed)
        self.cam_c = HR.make_camera(RES, CAM['camera_pos'], CAM['camera_lookat'], CAM['fov'], max_radius_px=CAM['max_radius_px'])
        self.cam_tiny_c = HR.make_camera(RES_TINY, CAM['camera_pos'], CAM['camera_lookat'], CAM['fov'], max_radius_px=CAM['max_radius_px'])
        self.lights_c = HR.make_lights(LIGHTS, ambient=AMBIENT)
        self.cam, self.cam_tiny, self.lights = RR.camera_of(self.cam_c), RR.camera_of(self.cam_tiny_c), RR.lights_of(self.lights_c)
        cam, (W, H) = self.cam, RES
        x = np.zeros((N, 3))
        used = np.ones(N, np.int32)
        k = 0
        self.sheet1 = np.arange(k, k + 230)                      # a jittered sheet at depth Z1
        for i in self.sheet1:
            x[i] = _at(cam, rng.uniform(8, 48), rng.uniform(10, 50), Z1 + rng.uniform(-0.01, 0.01))
        k += 230
        self.sheet2 = np.arange(k, k + 140)                      # a second one 0.3 behind it, overlapping it between columns 36 and 48
        for i in self.sheet2:
            x[i] = _at(cam, rng.uniform(36, 72), rng.uniform(14, 46), Z2 + rng.uniform(-0.01, 0.01))
        k += 140
        self.edge = np.arange(k, k + 12)                         # liquid discs across the four edges and the four corners
        spots = [(-0.3, 20.2), (W + 0.3, 9.4), (60.6, -0.4), (20.3, H + 0.4), (80.9, H - 0.3), (W - 0.2, 52.3), (-0.2, -0.2), (W + 0.1, -0.4), (-0.5, H + 0.3), (W + 0.2, H + 0.2),
                 (0.5, 0.5), (W - 0.5, H - 0.5)]
        for i, (px, py) in zip(self.edge, spots):
            x[i] = _at(cam, px, py, 1.2)
        k += 12
        self.lone = k                                            # far away and alone: a sub-pixel disc whose window holds nothing but itself
        x[k] = _at(cam, 85.5, 30.5, 8.0)
        k += 1
        self.unused = np.arange(k, k + 3)                        # selected, unused, where they would be seen
        for n, i in enumerate(self.unused):
            x[i] = _at(cam, 78.0 + 4 * n, 12.0, 0.9)
            used[i] = 0
        k += 3
        self.nonfinite = (k, k + 1)
        self.behind = k + 2
        k += 3
        self.spare = np.arange(k, N_LIQUID)                      # the rest of the selection thickens sheet 1
        for i in self.spare:
            x[i] = _at(cam, rng.uniform(8, 48), rng.uniform(10, 50), Z1 + rng.uniform(-0.01, 0.01))
        self.front = np.arange(N_LIQUID, N_LIQUID + 60)          # opaque, in front of sheet 1: they hide it
        for i in self.front:
            x[i] = _at(cam, rng.uniform(14, 30), rng.uniform(14, 30), rng.uniform(1.25, 1.35))
        self.back = np.arange(N_LIQUID + 60, N)                  # opaque, behind both sheets and beside them: seen through the liquid
        for i in self.back:
            x[i] = _at(cam, rng.uniform(4, 80), rng.uniform(6, 54), rng.uniform(2.2, 2.5))
        x = S.f32(x)
        x[self.nonfinite[0]] = S.f32(_at(cam, 80.0, 44.0, 0.9)); x[self.nonfinite[0], 1] = np.nan
        x[self.nonfinite[1]] = S.f32(_at(cam, 84.0, 44.0, 0.9)); x[self.nonfinite[1], 2] = np.inf
        x[self.behind] = S.f32(cam['pos'] - 0.5 * cam['fwd'])
        self.x, self.used, self.ids = x, used, np.arange(N)
        self.sel = np.zeros(N, np.uint8)
        self.sel[:N_LIQUID] = 1
        self.rgba = rng.randint(30, 256, (N, 4)).astype(np.uint8)
        self.rgba[:N_LIQUID // 2, :3] = (225, 228, 231)          # milk ...
        self.rgba[N_LIQUID // 2:N_LIQUID, :3] = (147, 107, 57)   # ... and coffee: the sheets mix both
        self.rgba[:, 3] = 255
        half = [_at(cam, rng.uniform(40, 60), rng.uniform(20, 28), rng.uniform(1.33, 1.37)) for _ in range(30)]      # a point set: in front of the liquid ...
        half += [_at(cam, rng.uniform(30, 70), rng.uniform(34, 44), rng.uniform(2.05, 2.15)) for _ in range(30)]     # ... and behind it
        self.tgt = S.f32(half)
        self.vol = sphere_volume()
        self._refs = {}

    def spheres(self, points=True):
        """(x, ids, radius, rgba, used-particle mask) of everything drawn as a sphere: the used particles, then the point set"""
        d = self.used != 0
        x, ids, rad, col = self.x[d], self.ids[d], np.full(d.sum(), R), self.rgba[d]
        if points:
            n = len(self.tgt)
            x, ids = np.concatenate([x, self.tgt]), np.concatenate([ids, N + np.arange(n)])
            rad, col = np.concatenate([rad, np.full(n, TGT_R)]), np.concatenate([col, np.tile(np.array(TGT_RGBA, np.uint8), (n, 1))])
        return x, ids, rad, col, d

    def ref(self, P, sel=None, tiny=False, points=True, volume=False):
        """the restatement's picture, computed once per case and left unchanged"""
        sel = self.sel if sel is None else np.asarray(sel, np.uint8)
        key = (tuple(sorted(P.items())), sel.tobytes(), tiny, points, volume)
        if key not in self._refs:
            x, ids, rad, col, d = self.spheres(points)
            liquid = np.zeros(len(x), bool)
            liquid[:d.sum()] = sel[d] != 0
            vols = [(VOL_SLOT, RS.volume(self.vol[0], self.vol[1], VOL_RGBA))] if volume else ()
            self._refs[key] = SR.render_surface(self.cam_tiny if tiny else self.cam, self.lights, N, x, ids, rad, col, liquid, P, volumes=vols)
        return self._refs[key]


def conditions(scene):
    """what the comparisons rest on, from the restatement alone; returns the figures it checked"""
    out = {}
    for iters, r in SWEEP + [(2, 5)]:
        ref = scene.ref(params(iters, r))
        n_liq, n_cov, n_fr = int(ref['liquid'].sum()), int(ref['covered'].sum()), int(ref['fragile'].sum())
        out[(iters, r)] = (n_liq, n_cov, n_fr)
        assert n_liq > 1000, (iters, r, n_liq)                   # (the sheets were laid out over 1,600 + 1,150 pixels)
        assert n_fr <= 0.005 * n_cov, (iters, r, n_fr, n_cov)
    ref = scene.ref(params(3, 8))
    liq, lid, op = ref['liquid'], ref['liq_id'], ref['opaque']
    seen = set(np.unique(lid[liq]).tolist())
    assert seen <= set(range(N_LIQUID))
    assert len(seen & set(scene.sheet1.tolist())) > 50 and len(seen & set(scene.sheet2.tolist())) > 30
    assert {int(c) for c in np.unique(scene.rgba[lid[liq], 0])} == {225, 147}                      # both colours
    for edge in (liq[:, 0], liq[:, -1], liq[0, :], liq[-1, :]):
        assert edge.sum() >= 2                                                                      # liquid on all four edges
    assert liq[0, 0] and liq[0, -1] and liq[-1, 0] and liq[-1, -1]                                  # ... and in all four corners
    jl, il = np.nonzero(lid == scene.lone)
    assert len(jl) == 1                                                                             # the lone particle: one pixel,
    win = liq[max(0, jl[0] - 8):jl[0] + 9, max(0, il[0] - 8):il[0] + 9]
    assert win.sum() == 1                                                                           # ... nothing else in its widest window,
    assert ref['z_smooth'][jl[0], il[0]] == ref['z_raw'][jl[0], il[0]]                              # ... so no pass moves it
    assert not seen & set(scene.unused.tolist()) and not seen & set(scene.nonfinite) and scene.behind not in seen
    # the opaque layer: particles in front hide the liquid, the ones behind show through it; the point set does both
    oid = op['id']
    assert (np.isin(oid, scene.front) & ~liq).sum() > 100 and (np.isin(oid, scene.back) & liq).sum() > 50
    assert ((oid >= N) & ~liq).sum() > 20 and ((oid >= N) & liq).sum() > 20
    assert not np.isin(ref['id'][liq], np.arange(N_LIQUID, N + len(scene.tgt))).any()
    # two sheets: both depths present, smoothed depths stay with their sheet (farther apart than `range`)
    zs = ref['z_smooth'][liq]
    near1, near2 = np.abs(zs - Z1) < 0.05, np.abs(zs - Z2) < 0.05
    assert near1.sum() > 500 and near2.sum() > 300
    # thickness: somewhere more than one sphere deep
    assert ref['thickness'].max() > 2.0 * 1.5 * R and (ref['thickness'][liq] > 0).all()
    # smoothing does something
    assert not np.array_equal(ref['z_smooth'], ref['z_raw'])
    # the picture differs from the spheres' and the liquid is translucent: what is behind changes the colour
    boxes = [RR.project(scene.cam, scene.x[i], 1.5 * R) for i in range(N_LIQUID) if scene.used[i]]
    px = [(b['i1'] - b['i0'] + 1) * (b['j1'] - b['j0'] + 1) for b in boxes if b is not None]
    assert sum(p > 25 for p in px) > 20 and sum(0 < p <= 25 for p in px) > 100                      # both roads at the default render_lane_pixels
    tiny = scene.ref(params(3, 8), tiny=True)
    assert tiny['liquid'].sum() >= 10 and int(tiny['fragile'].sum()) == 0
    out['tiny'] = (int(tiny['liquid'].sum()), int(tiny['covered'].sum()), int(tiny['fragile'].sum()))
    vol = scene.ref(params(2, 5), volume=True)
    vid = RS.vol_id0(N) + VOL_SLOT
    assert ((vol['opaque']['id'] == vid) & ~vol['liquid']).sum() > 50 and ((vol['opaque']['id'] == vid) & vol['liquid']).sum() > 50      # the volume hides liquid and shows through it
    assert int(vol['fragile'].sum()) <= 0.005 * int(vol['covered'].sum())
    out['volume'] = (int(vol['liquid'].sum()), int(vol['covered'].sum()), int(vol['fragile'].sum()))
    return out
