"""Liquids as a smoothed, translucent surface on the GPU (include/fluidengine_ext.h: fe_surface_*) against the numpy restatement of the contract
(tests/surface_ref.py) on the scene of tests/surface_cases.py: the liquid layer's ids, raw depth, thickness and smoothed depth and the
picture's depth and id bit for bit, RGB within one level outside the pixels the restatement calls fragile, on a 97 x 61 image and on a 7 x 5
one, for every smooth_iters in {0, 1, 3} and smooth_radius_px in {1, 8}; the lane road and the wave road; two draws; another particle order;
an empty selection against fe_render_scene_frame and fe_render_frame; everything selected; a volume in the opaque layer; a rollout that is
the same with and without surface pictures; every error; re-sizing; a second engine; LatteArt through env.render('rgb_array')."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import render_ref as RR  # noqa: E402
import scenarios as S  # noqa: E402
import surface_cases as SC  # noqa: E402
import surface_ref as SR  # noqa: E402
import test_render_hip as TR  # noqa: E402
from fluidlab_amd import _capi  # noqa: E402
from fluidlab_amd.fluidengine.renderers import hip_renderer as HR  # noqa: E402

pytestmark = pytest.mark.gpu

N, R = SC.N, SC.R
F_SORTED = 12                                                    # a frame behind the first sort (sort_interval 10): slot != pid
HUGE = 2 ** 31 - 1


@pytest.fixture(scope='module')
def scene():
    sc = SC.Scene()
    SC.conditions(sc)                                            # (the conditions on the scene come before any comparison)
    return sc


def _engine(hiplib, scene, x=None, used=None, rgba=None, steps=F_SORTED):
    eng = S.make_engine(hiplib, S.water_block(n_grid=16, n_particles=N), max_substeps_local=32)
    if steps:
        eng.step(0, 0, steps, 0)
        eng.set_frame(steps, x=scene.x if x is None else x, used=scene.used if used is None else used)
    eng.set_frame(0, x=scene.x if x is None else x, used=scene.used if used is None else used)
    eng.render_setup(scene.cam_c, scene.lights_c)
    eng.render_set_colors(scene.rgba if rgba is None else rgba, R)
    eng.render_set_points(0, scene.tgt, SC.TGT_RGBA, SC.TGT_R)
    return eng


@pytest.fixture(scope='module')
def drawn(hiplib, scene):
    """an engine stepped past its first sort, the scene written over frame F_SORTED (sorted slots) and frame 0 (identity order)"""
    eng = _engine(hiplib, scene)
    assert eng.get_option('sort_interval') == 10 and eng.get_option('render_lane_pixels') == _capi.FE_RENDER_LANE_PIXELS
    yield eng
    eng.close()


def _draw(eng, f=F_SORTED, s=0):
    """(rgba, depth, id, z_raw, z_smooth, thickness) of the surface picture of frame f"""
    eng.surface_frame(f, s)
    return eng.render_get(True, True, True) + eng.surface_get()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(a, b))


def _check(ref, pic):
    rgba, depth, ids, z_raw, z_smooth, thick = pic
    assert np.all(rgba[..., 3] == 255)
    liq = ref['liquid']
    assert np.array_equal(np.isfinite(z_raw), liq)
    assert np.array_equal(ids[liq], ref['liq_id'][liq])          # the liquid layer's ids, bit for bit
    bad = SR.compare(ref, rgba, depth, ids, z_raw, z_smooth, thick)
    assert not bad, bad
    return int((rgba[..., :3] == ref['rgb']).all(-1).sum())


@pytest.mark.parametrize('iters,r', SC.SWEEP + [(2, 5)])
def test_picture_against_the_restatement(drawn, scene, iters, r):
    P = SC.params(iters, r)
    drawn.surface_set(scene.sel, SC.params_c(P))
    pic = _draw(drawn)
    assert pic[0].shape == (61, 97, 4) and pic[3].dtype == np.float32 and pic[5].dtype == np.float64
    exact = _check(scene.ref(P), pic)
    print(f'iters {iters} r {r}: rgb equal on {exact} of {61 * 97} pixels')
    if iters == 0:
        assert np.array_equal(pic[3].view(np.uint32), pic[4].view(np.uint32))       # no pass: the smoothed depth is the raw one


@pytest.mark.parametrize('iters,r', [(1, 1), (3, 8)])
def test_an_image_smaller_than_one_tile(drawn, scene, iters, r):
    P = SC.params(iters, r)
    drawn.surface_set(scene.sel, SC.params_c(P))
    drawn.render_setup(scene.cam_tiny_c, scene.lights_c)         # the images follow the renderer's size
    try:
        pic = _draw(drawn)
        assert pic[0].shape == (5, 7, 4) and pic[4].shape == (5, 7)
        _check(scene.ref(P, tiny=True), pic)
    finally:
        drawn.render_setup(scene.cam_c, scene.lights_c)
    _check(scene.ref(P), _draw(drawn))                           # ... and back


def test_roads_and_repeats_give_the_same_bytes(drawn, scene):
    drawn.surface_set(scene.sel, SC.params_c(SC.params(3, 8)))
    base = _draw(drawn)
    assert _same(base, _draw(drawn))                             # two draws
    try:
        for lane_pixels in (0, HUGE, 7):                         # wave only, lane only, a split elsewhere
            drawn.set_option('render_lane_pixels', lane_pixels)
            assert _same(base, _draw(drawn)), f'render_lane_pixels = {lane_pixels}'
    finally:
        drawn.set_option('render_lane_pixels', _capi.FE_RENDER_LANE_PIXELS)
    assert _same(base, _draw(drawn, 0))                          # the same states in the slots of the identity order


def test_another_particle_order_gives_the_same_picture(drawn, scene, hiplib):
    P = SC.params(3, 8)
    drawn.surface_set(scene.sel, SC.params_c(P))
    base = _draw(drawn)
    perm = np.random.RandomState(3).permutation(N)               # new particle p is old particle perm[p]
    eng = _engine(hiplib, scene, scene.x[perm], scene.used[perm], scene.rgba[perm], steps=0)
    eng.surface_set(scene.sel[perm], SC.params_c(P))
    pic = _draw(eng, 0)
    eng.close()
    assert _same((base[0], base[1]) + base[3:], (pic[0], pic[1]) + pic[3:])          # colour, depth and the layer's images stay
    old = np.where((pic[2] >= 0) & (pic[2] < N), perm[np.clip(pic[2], 0, N - 1)], pic[2])
    assert np.array_equal(old, base[2])                          # ... and the ids are the permuted ones (point-set ids as they were)


def test_an_empty_selection_is_the_opaque_picture(drawn, scene):
    P = SC.params_c(SC.params(3, 8))
    drawn.render_scene_frame(F_SORTED, 0)
    plain = drawn.render_get(True, True, True)
    drawn.render_frame(F_SORTED)
    assert _same(plain, drawn.render_get(True, True, True))     # (no scene is set: the same picture)
    for sel in (None, np.zeros(N, np.uint8)):
        drawn.surface_set(sel, P)
        drawn.surface_frame(F_SORTED, 0)
        assert _same(plain, drawn.render_get(True, True, True))
        with pytest.raises(Exception, match='no surface picture'):
            drawn.surface_get()
    ref = scene.ref(SC.params(3, 8), sel=np.zeros(N, np.uint8))
    assert not RR.compare(dict(ref, id2=ref['id']), *plain)
    # with a volume in the scene: still exactly fe_render_scene_frame, and with the selection the volume belongs to the opaque layer
    drawn.render_set_volume(SC.VOL_SLOT, _capi.FE_RENDER_VOL_OWN, 0, SC.VOL_RGBA, *scene.vol)
    try:
        drawn.render_scene_frame(F_SORTED, 0)
        with_vol = drawn.render_get(True, True, True)
        assert not _same(plain, with_vol)
        drawn.surface_frame(F_SORTED, 0)
        assert _same(with_vol, drawn.render_get(True, True, True))
        P = SC.params(2, 5)
        drawn.surface_set(scene.sel, SC.params_c(P))
        _check(scene.ref(P, volume=True), _draw(drawn))
    finally:
        drawn.render_set_volume(SC.VOL_SLOT)


def test_everything_selected(drawn, scene):
    P = SC.params(1, 8)
    sel = np.ones(N, np.uint8)
    drawn.surface_set(sel, SC.params_c(P))
    ref = scene.ref(P, sel=sel)
    assert ref['liquid'].sum() > 1000 and int(ref['fragile'].sum()) <= 0.005 * int(ref['covered'].sum())
    pic = _draw(drawn)
    _check(ref, pic)
    assert set(np.unique(pic[2]).tolist()) - set(range(-1, N)) <= set(range(N, N + len(scene.tgt)))      # only the point set is opaque


def _rollout(hiplib, scene, surface):
    """tests/test_render_hip.py's injector rollout (latte_mini, 32 substeps one by one, sorts at 10, 20, 30) with a surface picture of every new
    frame instead of a particle picture"""
    sc = S.latte_mini(horizon=8)
    inj = sc['injector']
    eng = S.make_engine(hiplib, sc)
    eng.profile_enable(True)
    e = eng.add_effector(type=S.FE_EFF_INJECTOR, action_dim=inj['action_dim'], action_scale_v=inj['action_scale_v'],
                         action_scale_p=inj['action_scale_p'], boundary=hiplib.make_boundary(**inj['boundary']),
                         flux=inj['flux'], radius=inj['radius'], inject_v=inj['inject_v'], inject_p=inj['inject_p'],
                         locally_random=inj['locally_random'], random_vector=inj['random_vector'])
    eng.eff_set_act_range(e, np.where(sc['used'] == 0)[0].astype(np.int32))
    st0 = eng.eff_get_state(e, 0)
    st0[:7] = [0.5, 0.5, 0.5, 1.0, 0.0, 0.0, 0.0]
    eng.eff_set_state(e, 0, st0)
    eng.eff_apply_action_p(e, sc['action_p'])
    ns, H = sc['n_substeps'], sc['horizon']
    n_liquid, touched = [], 0
    if surface:
        eng.render_setup(scene.cam_c, scene.lights_c)
        eng.render_set_colors(np.full((sc['N'], 4), 200, np.uint8), 0.02)
        sel = np.zeros(sc['N'], np.uint8)
        sel[::2] = 1                                             # half of the particles, pool and coffee alike
        eng.surface_set(sel, SC.params_c(SR.params(range=0.2)))
    for s in range(H):
        eng.eff_set_action(e, s, s, ns, sc['actions'][s])
        for k in range(ns):
            f = s * ns + k
            eng.substep(f, f, 1)
            if surface:
                before = TR._frame_words(eng, f + 1)
                pic = _draw(eng, f + 1)
                after = TR._frame_words(eng, f + 1)
                touched += any(not np.array_equal(before[w], after[w]) for w in before)
                n_liquid.append(int(np.isfinite(pic[3]).sum()))
    launches = {k: n for k, (ms, n) in eng.profile_read().items()}
    frames = [TR._frame_words(eng, f, with_F=True) for f in range(ns * H + 1)]
    if surface:                                                  # every stored frame once more, behind the expansion of F: still only read
        for f in range(ns * H + 1):
            _draw(eng, f)
        touched += sum(any(not np.array_equal(a[w], b[w]) for w in a) for a, b in zip(frames, [TR._frame_words(eng, f, with_F=True) for f in range(ns * H + 1)]))
    eng.close()
    return frames, n_liquid, launches, touched


def test_surface_pictures_leave_the_rollout_as_it_is(hiplib, scene):
    """The method of tests/test_render_hip.py (its docstring says why the plain rollout runs twice): equal word for word wherever two plain runs
    are equal, beyond that `used` equal and x, v, C, F no farther from the plain run than 4 x what the two plain runs lie apart plus that
    test's few ulp; the same substep kernels launched; no picture changes a word of any frame."""
    with_surface, n_liquid, launches_s, touched = _rollout(hiplib, scene, True)
    plain, _, launches_p, _ = _rollout(hiplib, scene, False)
    plain2, _, _, _ = _rollout(hiplib, scene, False)
    assert len(with_surface) == len(plain) == len(plain2) == 33
    (f_noise, noise), (f_diff, diff) = TR._first_difference(plain, plain2), TR._first_difference(plain, with_surface)
    print(f'plain against plain: first difference {noise}; plain against surface pictures: first difference {diff}; pictures that changed a frame: {touched}')
    assert touched == 0
    assert launches_s == launches_p and sum(launches_p.values()) > 0, (launches_s, launches_p)
    assert f_noise >= 2, noise
    assert f_diff >= f_noise, (diff, noise)
    for f in range(f_noise, 33):
        r, p, q = with_surface[f], plain[f], plain2[f]
        assert np.array_equal(r['used'], p['used']) and np.array_equal(q['used'], p['used']), f
        u = p['used'].view(np.int32) != 0
        for k in 'xvCF':
            d, nz = TR._apart(r, p, k, u), TR._apart(q, p, k, u)
            assert d <= 4.0 * nz + {'x': 5e-7, 'v': 4e-6, 'C': 8e-5, 'F': 4e-6}[k], (f, k, d, nz)
    assert min(n_liquid) > 50                                    # the pictures showed liquid


def test_errors_leave_the_previous_state(drawn, scene, hiplib):
    eng, lib, h = drawn, drawn.lib, drawn.h
    P = SC.params(3, 8)
    eng.surface_set(scene.sel, SC.params_c(P))
    before = _draw(eng)

    def keep(call, match):
        with pytest.raises(Exception, match=match):
            call()
        assert _same(before, _draw(eng)), match

    def with_(**kw):
        c = SC.params_c(P)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    sel = np.ascontiguousarray(scene.sel)
    other = np.ascontiguousarray(1 - scene.sel)                  # (a refused call must not take this selection either)
    nan, inf = float('nan'), float('inf')
    for size in (C.sizeof(_capi.FeSurfaceParams) - 8, C.sizeof(_capi.FeSurfaceParams) + 8, 0):
        keep(lambda: eng._ck(lib.fe_surface_set(h, other.ctypes.data_as(C.c_void_p), C.byref(SC.params_c(P)), size)), 'FeSurfaceParams size')
    keep(lambda: eng._ck(lib.fe_surface_set(h, other.ctypes.data_as(C.c_void_p), None, C.sizeof(_capi.FeSurfaceParams))), 'FeSurfaceParams size')
    bad = [('radius_scale', (0.99, 0.0, -2.0, nan, inf)), ('smooth_iters', (-1, 9)), ('smooth_radius_px', (0, 9, -3)), ('range', (0.0, -0.1, nan, inf)),
           ('absorb', (-1e-9, nan, inf)), ('alpha_min', (-0.01, 1.01, nan)), ('specular', (-0.01, 1.01, nan, inf)), ('shininess_log2', (-1, 11))]
    for name, values in bad:
        for v in values:
            keep(lambda: eng.surface_set(other, with_(**{name: v})), name)
    for f in (-1, 33, 10 ** 6):
        keep(lambda: eng.surface_frame(f), 'frame index out of range')
    eng.surface_set(sel, with_(radius_scale=1e9))                # in range, but 2 R_s N no longer fits a thickness word: the frame is refused,
    with pytest.raises(Exception, match='too large for the thickness words'):
        eng.surface_frame(F_SORTED)
    assert _same(before, eng.render_get(True, True, True) + eng.surface_get())      # ... nothing was drawn over the last picture
    eng.surface_set(scene.sel, SC.params_c(P))
    assert _same(before, _draw(eng))
    # before setup, before colours, before a picture
    fresh = S.make_engine(hiplib, S.water_block(n_grid=16, n_particles=64), max_substeps_local=4)
    some = np.ones(64, np.uint8)
    for call in (lambda: fresh.surface_set(some, SC.params_c(P)), lambda: fresh.surface_set(None), lambda: fresh.surface_frame(0),
                 lambda: fresh._ck(fresh.lib.fe_surface_get(fresh.h, None, None, None)), lambda: fresh._ck(fresh.lib.fe_surface_get_dev(fresh.h, None, None, None))):
        with pytest.raises(Exception, match='fe_render_setup first'):
            call()
    fresh.render_setup(scene.cam_c, scene.lights_c)
    bytes0 = fresh.get_stats(0)['bytes_state']
    fresh.surface_set(None)
    fresh.surface_set(np.zeros(64, np.uint8), SC.params_c(P))
    assert fresh.get_stats(0)['bytes_state'] == bytes0           # nothing is allocated before a selection that is not empty
    fresh.surface_set(some, SC.params_c(P))
    assert fresh.get_stats(0)['bytes_state'] > bytes0
    with pytest.raises(Exception, match='fe_render_set_colors first'):
        fresh.surface_frame(0)
    with pytest.raises(Exception, match='no surface picture'):
        fresh.surface_get()
    fresh.render_set_colors(np.full((64, 4), 200, np.uint8), 0.02)
    fresh.surface_frame(0)
    z = fresh.surface_get()[0]
    assert np.isfinite(z).any()
    fresh.render_setup(scene.cam_c, scene.lights_c)              # a new setup: the old picture is gone
    with pytest.raises(Exception, match='no surface picture'):
        fresh.surface_get()
    fresh.close()
    # a second engine after the first was destroyed, and one without particles
    again = S.make_engine(hiplib, S.water_block(n_grid=16, n_particles=64), max_substeps_local=4)
    again.render_setup(scene.cam_c, scene.lights_c)
    again.render_set_colors(np.full((64, 4), 200, np.uint8), 0.02)
    again.surface_set(some, SC.params_c(P))
    again.surface_frame(0)
    assert np.array_equal(np.isfinite(again.surface_get()[0]), np.isfinite(z))
    again.close()
    assert _same(before, _draw(eng))


def test_device_copies(drawn, scene):
    import torch
    drawn.surface_set(scene.sel, SC.params_c(SC.params(3, 8)))
    pic = _draw(drawn)
    dev = f'cuda:{drawn.device}'
    z_raw, z_smooth = torch.empty((61, 97), dtype=torch.float32, device=dev), torch.empty((61, 97), dtype=torch.float32, device=dev)
    thick = torch.empty((61, 97), dtype=torch.float64, device=dev)
    drawn.surface_get_dev(z_raw, z_smooth, thick)
    drawn.sync()
    assert _same(pic[3:], (z_raw.cpu().numpy(), z_smooth.cpu().numpy(), thick.cpu().numpy()))
    with pytest.raises(_capi.FeEngineError, match='thickness must be'):
        drawn.surface_get_dev(thickness=torch.empty((61, 97), dtype=torch.float32, device=dev))


def test_latteart_env_draws_its_liquids_as_a_surface(hiplib):
    from fluidlab_amd.envs import make
    from fluidlab_amd.configs.macros import MAT_CLASS, MAT_LIQUID
    import test_hip_env as E
    import test_render_scene_hip as TS
    env = make('LatteArt-v0', seed=0, loss=False, renderer_type='HIP', **E.MINI)
    te = env.taichi_env
    r, sim = te.renderer, te.simulator
    TS._small_picture(te)                                        # the environment's own camera at 160 x 160: the restatement is numpy
    env.reset()
    action = np.full(env.action_space.shape, 0.004, np.float32)
    for _ in range(3):
        te.step(action)
    spheres = te.render_buffers()                                # today's picture
    n = sim.n_particles
    x = np.zeros((n, 3), np.float32); used = np.zeros((n,), np.int32)
    sim.engine.get_frame(sim.cur_substep_local, x=x, used=used)
    d = used != 0
    rgba = HR.colors_to_bytes(te.particles['color'])
    cam, lights = RR.camera_of(r.camera), RR.lights_of(r.lights)
    assert not RR.compare(RR.render(cam, lights, x[d], np.arange(n)[d], r.particle_radius, rgba[d]), *[np.concatenate([spheres[0], np.full((160, 160, 1), 255, np.uint8)], -1), spheres[1], spheres[2]])
    env.enable_liquid_surface()
    assert r.surface_enabled and r.surface.radius_scale == 1.5 and r.surface.smooth_iters == 2 and r.surface.smooth_radius_px == 5
    liquid = np.array([MAT_CLASS[int(m)] == MAT_LIQUID for m in sim.engine.get_mat()])
    assert np.array_equal(r.surface_selection, liquid) and liquid.all()           # LatteArt is milk on coffee: everything is liquid
    rgb, depth, ids = te.render_buffers()
    assert np.array_equal(env.render('rgb_array'), rgb)
    z_raw, z_smooth, thick = te.render_surface_buffers()
    ref = SR.render_surface(cam, lights, n, x[d], np.arange(n)[d], r.particle_radius, rgba[d], liquid[d], SR.params_of(r.surface))
    n_cov, n_fr = int(ref['covered'].sum()), int(ref['fragile'].sum())
    print(f'LatteArt surface: liquid {int(ref["liquid"].sum())} covered {n_cov} fragile {n_fr}')
    assert ref['liquid'].sum() > 2000
    bad = SR.compare(ref, np.concatenate([rgb, np.full((160, 160, 1), 255, np.uint8)], -1), depth, ids, z_raw, z_smooth, thick)
    assert not bad, bad
    assert not np.array_equal(rgb, spheres[0])                   # it differs from the sphere picture,
    r.disable_liquid_surface()
    assert _same(spheres, te.render_buffers())                   # ... and without the surface the picture is today's, byte for byte
    sim.engine.close()
