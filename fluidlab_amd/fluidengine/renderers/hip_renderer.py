"""HIPRenderer -- the headless particle renderer (include/fluidengine_ext.h: fe_render_*), with the keywords of the reference's
GGUIRenderer (fluidengine/renderers/ggui_renderer.py): every used particle is a sphere in its body's colour, target particles and markers
are static point sets.  enable_scene() adds what the fluid touches: the SDF colliders of statics and Rigid effectors, drawn from the voxel
blocks the engine collides with (there are no triangle meshes here), and the smoke field as one sphere per cell of its visible slab
(smoke_field.py:28-31, 292-299).  enable_liquid_surface() draws the liquid particles as one smoothed, translucent surface over all that.
Nothing else is transparent, and there is no window.  The camera basis is built here in fp64; the engine does no trigonometry."""
import numpy as np

from fluidlab_amd import _capi
from fluidlab_amd.configs.macros import COLOR, MAT_CLASS, MAT_LIQUID, TARGET
from fluidlab_amd.fluidengine.effectors.rigid import Rigid

#: target particles are drawn in COLOR[TARGET] (ggui_renderer.py:163-166), opaque
TARGET_RGBA = tuple(int(c * 255.0 + 0.5) for c in COLOR[TARGET][:3]) + (255,)
#: the lights of ggui_renderer.py:19-20
#: the smoke field's colours (smoke_field.py:28-31)
SMOKE_HOT, SMOKE_COLD = (1.0, 0.45, 0.14), (0.0, 0.55, 1.0)
#: enable_liquid_surface(): chosen by eye, not measured.  range 0 stands for four liquid radii (4 radius_scale particle_radius).
LIQUID_SURFACE_DEFAULTS = dict(radius_scale=1.5, smooth_iters=2, smooth_radius_px=5, range=0.0, absorb=40.0, alpha_min=0.25, specular=0.3, shininess_log2=5)
DEFAULT_LIGHTS = ({'pos': (0.5, 1.5, 0.5), 'color': (0.5, 0.5, 0.5)}, {'pos': (0.5, 1.5, 1.5), 'color': (0.5, 0.5, 0.5)})


def camera_basis(camera_pos, camera_lookat, up=(0.0, 1.0, 0.0)):
    """(right, up, fwd): an orthonormal basis looking from camera_pos to camera_lookat, fp64"""
    pos, at, up = (np.asarray(v, np.float64) for v in (camera_pos, camera_lookat, up))
    fwd = at - pos
    n = np.linalg.norm(fwd)
    if not n > 0:
        raise ValueError('camera_pos and camera_lookat coincide')
    fwd = fwd / n
    right = np.cross(fwd, up)
    n = np.linalg.norm(right)
    if not n > 1e-12:
        raise ValueError('the view direction is parallel to `up`')
    right = right / n
    return right, np.cross(right, fwd), fwd


def make_camera(res, camera_pos, camera_lookat, fov, up=(0.0, 1.0, 0.0), near=0.01, max_radius_px=32.0):
    """the FeRenderCamera of a width x height image with a vertical field of view of `fov` degrees"""
    W, H = int(res[0]), int(res[1])
    right, upv, fwd = camera_basis(camera_pos, camera_lookat, up)
    cam = _capi.FeRenderCamera()
    cam.pos[:] = [float(v) for v in camera_pos]
    cam.right[:] = [float(v) for v in right]
    cam.up[:] = [float(v) for v in upv]
    cam.fwd[:] = [float(v) for v in fwd]
    cam.focal = float(0.5 * H / np.tan(np.deg2rad(float(fov)) / 2.0))
    cam.near, cam.max_radius_px = float(near), float(max_radius_px)
    cam.width, cam.height = W, H
    return cam


def make_lights(lights, ambient=(0.1, 0.1, 0.1), background=(1.0, 1.0, 1.0)):
    if len(lights) > _capi.FE_RENDER_MAX_LIGHTS:
        raise ValueError(f'at most {_capi.FE_RENDER_MAX_LIGHTS} lights')
    L = _capi.FeRenderLights()
    L.ambient[:] = [float(v) for v in ambient]
    L.background[:] = [float(v) for v in background]
    for k, light in enumerate(lights):
        L.pos[k][:] = [float(v) for v in light['pos']]
        L.color[k][:] = [float(v) for v in light['color']]
    L.n_lights = len(lights)
    return L


def colors_to_bytes(color):
    """float RGBA in [0, 1] (Bodies' particles['color']) or uint8 -> uint8 [n, 4]"""
    c = np.asarray(color)
    if c.dtype == np.uint8:
        return np.ascontiguousarray(c.reshape(-1, 4))
    return np.ascontiguousarray((np.clip(c.astype(np.float64), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8).reshape(-1, 4))


class HIPRenderer:
    def __init__(self, res=(640, 640), camera_pos=(0.5, 2.5, 3.5), camera_lookat=(0.5, 0.5, 0.5), fov=30, particle_radius=0.0075,
                 lights=DEFAULT_LIGHTS,
                 background=(1.0, 1.0, 1.0), ambient=(0.1, 0.1, 0.1), up=(0.0, 1.0, 0.0), near=0.01, max_radius_px=32.0):
        self.res = (int(res[0]), int(res[1]))
        self.particle_radius = float(particle_radius)
        self.camera = make_camera(self.res, camera_pos, camera_lookat, fov, up, near, max_radius_px)
        self.lights = make_lights(list(lights), ambient, background)
        self.engine = self.sim = None
        self._has_target = False
        self.scene_enabled = False
        self.surface_enabled = False                            # enable_liquid_surface(): liquids as a translucent surface
        self.volumes = []                                       # enable_scene(): (slot, 'static' | 'effector' | 'own', index, rgba) of every volume drawn

    def build(self, sim, particles):
        """after the simulator: the engine exists.  particles: Bodies.get() (its 'color' is uploaded); a scene without particles draws point sets only"""
        self.engine, self.sim = sim.engine, sim
        if not self.engine.elib.has_ext:
            raise _capi.FeEngineError(f'render calls are not available on {self.engine.elib.backend}')
        self.engine.render_setup(self.camera, self.lights)
        n = self.engine.N
        rgba = colors_to_bytes(particles['color']) if particles is not None else np.zeros((n, 4), np.uint8)
        self.engine.render_set_colors(rgba, self.particle_radius)

    def set_target(self, tgt_particles, rgba=TARGET_RGBA, radius=None):
        """the reference's tgt_particles: point set 0 (None removes it)"""
        if tgt_particles is None:
            if self._has_target:
                self.engine.render_set_points(0, None)
                self._has_target = False
            return
        self.engine.render_set_points(0, tgt_particles, rgba, self.particle_radius if radius is None else radius)
        self._has_target = True

    def set_markers(self, xyz, rgba=(40, 40, 230, 255), radius=None):
        """markers such as an effector's position: point set 1 (None removes it)"""
        self.engine.render_set_points(1, xyz, rgba, 2.0 * self.particle_radius if radius is None else radius)

    def _take_volume(self, what, source, index, color, voxels=None, T=None):
        if color[3] < 1.0:
            print(f'HIPRenderer: {what} is transparent (alpha {color[3]:g}) and only liquids are drawn translucent: not drawn')
            return
        slot = len(self.volumes)
        if slot >= _capi.FE_RENDER_MAX_VOLUMES:
            print(f'HIPRenderer: {what}: all {_capi.FE_RENDER_MAX_VOLUMES} volume slots are taken: not drawn')
            return
        rgba = tuple(int(c) for c in colors_to_bytes(np.asarray([color], np.float64))[0])
        self.engine.render_set_volume(slot, source, index, rgba, voxels, T)
        self.volumes.append((slot, {_capi.FE_RENDER_VOL_STATIC: 'static', _capi.FE_RENDER_VOL_EFFECTOR: 'effector', _capi.FE_RENDER_VOL_OWN: 'own'}[source], index, rgba))

    def enable_scene(self, statics=True, effectors=True, smoke=True, march_step=0.5, bisect_iters=10):
        """After build(): from here on the pictures show the scene's colliders -- the engine's statics, every Rigid effector with a mesh, and a
        visual-only static (has_dynamics=False) where an SDF can be had for it -- in COLOR[material], and the smoke field of a scene that has
        one.  A collider whose colour has alpha < 1 (TANK, BOTTLE) is skipped: only liquids are drawn translucent."""
        if self.engine is None:
            raise RuntimeError('enable_scene: build() first')
        for slot, _, _, _ in self.volumes:
            self.engine.render_set_volume(slot)
        self.volumes = []
        sim = self.sim
        if statics and getattr(sim, 'statics', None) is not None:
            i_engine = 0
            for k, st in enumerate(sim.statics):
                what = f'static {k} ({st.raw_file})'
                if st.has_dynamics:
                    self._take_volume(what, _capi.FE_RENDER_VOL_STATIC, i_engine, COLOR[st.material])
                    i_engine += 1
                    continue
                if not hasattr(st, 'sdf_voxels_np'):
                    if st._sdf_arg is None and not st._asset_present():
                        print(f'HIPRenderer: {what} is visual only and has neither a mesh in the asset tree nor an sdf= stand-in: not drawn')
                        continue
                    st._prepared = False
                    st.prepare(self.engine.elib, self.engine.device)
                self._take_volume(what, _capi.FE_RENDER_VOL_OWN, 0, COLOR[st.material], st.sdf_voxels_np.astype(self.engine.dtype), st.T_mesh_to_voxels_np)
        if effectors and getattr(sim, 'agent', None) is not None:
            for e in sim.agent.effectors:
                if isinstance(e, Rigid) and e.mesh is not None:
                    self._take_volume(f'effector {e.index} ({e.mesh.raw_file})', _capi.FE_RENDER_VOL_EFFECTOR, e.index, COLOR[e.mesh.material])
        sc = _capi.FeRenderScene()
        sc.march_step, sc.bisect_iters = float(march_step), int(bisect_iters)
        sf = getattr(sim, 'smoke_field', None)
        if smoke and sf is not None:
            sc.draw_smoke, sc.lo, sc.hi, sc.smoke_radius = 1, int(sf.lower_y), int(sf.higher_y), 1.0 / sf.n_grid
            sc.cold[:], sc.hot[:] = SMOKE_COLD, SMOKE_HOT
        self.engine.render_set_scene(sc)
        self.scene = sc
        self.scene_enabled = True

    def enable_liquid_surface(self, materials=None, selection=None, **params):
        """After build(): from here on the liquid particles are drawn as one smoothed, translucent surface over the rest of the picture
        (include/fluidengine_ext.h: fe_surface_*).  By default every particle whose material class is MAT_LIQUID is liquid -- the rule of the
        reference's GL renderer (gl_renderer.py:71-105, bodies_needs_smoothing); `materials` names the material ids instead, `selection` a
        bool array [N] by particle id.  The keywords are FeSurfaceParams' fields; the defaults (LIQUID_SURFACE_DEFAULTS) were chosen by eye on
        LatteArt-v0 and Pouring-v0 pictures, not measured against anything.  An empty selection switches the surface off."""
        if self.engine is None:
            raise RuntimeError('enable_liquid_surface: build() first')
        unknown = set(params) - set(LIQUID_SURFACE_DEFAULTS)
        if unknown:
            raise TypeError(f'enable_liquid_surface: unknown keyword(s) {sorted(unknown)}')
        if selection is None:
            mat = np.asarray(self.engine.get_mat()).reshape(-1)
            ids = [m for m, c in MAT_CLASS.items() if c == MAT_LIQUID] if materials is None else [int(m) for m in materials]
            selection = np.isin(mat, ids)
        selection = np.asarray(selection).reshape(-1) != 0
        p = _capi.FeSurfaceParams()
        for k, v in {**LIQUID_SURFACE_DEFAULTS, **params}.items():
            setattr(p, k, v)
        if p.range <= 0.0:                                       # the default: four liquid radii
            p.range = 4.0 * p.radius_scale * self.particle_radius
        self.engine.surface_set(selection, p)
        self.surface, self.surface_selection = p, selection
        self.surface_enabled = bool(selection.any())

    def disable_liquid_surface(self):
        if self.engine is not None and self.surface_enabled:
            self.engine.surface_set(None)
        self.surface_enabled = False

    def render_surface_buffers(self, f, tgt_particles=None):
        """(z_raw float32 [H, W], z_smooth float32 [H, W], thickness float64 [H, W]) of the liquid layer of frame f: +inf / 0 where no liquid is"""
        if not self.surface_enabled:
            raise RuntimeError('render_surface_buffers: enable_liquid_surface() first (with a selection that is not empty)')
        self.set_target(tgt_particles)
        self._draw(f)
        return self.engine.surface_get()

    def _draw(self, f):
        if self.surface_enabled:
            self.engine.surface_frame(f, self.sim.cur_step_local if self.scene_enabled and self.scene.draw_smoke else 0)
        elif self.scene_enabled:
            self.engine.render_scene_frame(f, self.sim.cur_step_local if self.scene.draw_smoke else 0)
        else:
            self.engine.render_frame(f)

    def render_frame(self, f, tgt_particles=None):
        """uint8 [H, W, 3] of frame f"""
        self.set_target(tgt_particles)
        self._draw(f)
        rgba, _, _ = self.engine.render_get()
        return np.ascontiguousarray(rgba[:, :, :3])

    def render_buffers(self, f, tgt_particles=None):
        """(rgb uint8 [H, W, 3], depth float32 [H, W] with +inf on background, id int32 [H, W] with -1 on background)"""
        self.set_target(tgt_particles)
        self._draw(f)
        rgba, depth, ids = self.engine.render_get(True, True, True)
        return np.ascontiguousarray(rgba[:, :, :3]), depth, ids

    def render_dev(self, f, tgt_particles=None):
        """the RGBA image of frame f as a torch uint8 tensor [H, W, 4] on the engine's GPU; nothing crosses PCIe"""
        import torch
        self.set_target(tgt_particles)
        W, H = self.res
        out = torch.empty((H, W, 4), dtype=torch.uint8, device=f'cuda:{self.engine.device}')
        self._draw(f)
        self.engine.render_get_dev(rgba=out)
        self.engine.sync()
        return out
