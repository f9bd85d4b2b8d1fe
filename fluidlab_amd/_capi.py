"""ctypes binding of the FluidEngine C ABI (include/fluidengine.h).

`load_hip()` is the product entry: it loads the in-tree gfx950 library
`fluidlab_amd/csrc/libfluidengine_hip.so` and raises if it is missing -- there is
no CPU fallback.  `EngineLib(path)` binds any library exporting the same ABI; the
tests use that to drive the host logic with the oracle build (tests only).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.path.join(_HERE, 'csrc', 'libfluidengine_hip.so')

FE_BOUNDARY_CUBE, FE_BOUNDARY_CYLINDER = 0, 1
FE_EFF_PLAIN, FE_EFF_INJECTOR, FE_EFF_AIRCON = 0, 1, 2


class FeEngineError(RuntimeError):
    pass


def _structs(real):
    class FeBoundary(C.Structure):
        _fields_ = [('type', C.c_int), ('lower', real * 3), ('upper', real * 3),
                    ('xz_center', real * 2), ('xz_radius', real), ('restitution', real),
                    ('lock_dims', C.c_int)]

    class FeConfig(C.Structure):
        _fields_ = [('struct_size', C.c_int), ('n_grid', C.c_int), ('n_particles', C.c_int),
                    ('max_substeps_local', C.c_int), ('n_substeps', C.c_int),
                    ('max_action_steps', C.c_int), ('dt', real), ('p_vol', real),
                    ('gravity', real * 3), ('boundary', FeBoundary), ('device', C.c_int)]

    class FeEffectorDesc(C.Structure):
        _fields_ = [('struct_size', C.c_int), ('type', C.c_int), ('action_dim', C.c_int),
                    ('action_scale_v', real * 8), ('action_scale_p', real * 8),
                    ('boundary', FeBoundary), ('flux', C.c_int), ('radius', real),
                    ('inject_v', real * 3), ('inject_p', real * 3),
                    ('locally_random', C.c_int), ('randomize_inject_v', C.c_int),
                    ('random_length', C.c_int)]

    class FeSdfDesc(C.Structure):
        _fields_ = [('struct_size', C.c_int), ('res', C.c_int), ('T_mesh_to_voxels', real * 16),
                    ('friction', real), ('softness', real)]

    class FeSmokeConfig(C.Structure):
        _fields_ = [('struct_size', C.c_int), ('res', C.c_int), ('solver_iters', C.c_int), ('q_dim', C.c_int),
                    ('max_steps_local', C.c_int), ('dt', real), ('decay', real), ('high_T', real), ('low_T', real),
                    ('lower_y', C.c_int), ('higher_y', C.c_int)]

    return FeBoundary, FeConfig, FeEffectorDesc, FeSdfDesc, FeSmokeConfig


class FeStats(C.Structure):
    _fields_ = [('n_used', C.c_longlong), ('n_cells_touched', C.c_longlong),
                ('n_blocks_active', C.c_longlong), ('n_slow_path', C.c_longlong),
                ('bytes_state', C.c_longlong)]


class FeFrameSummary(C.Structure):
    """include/fluidengine_ext.h: one group's (or the whole frame's) record of fe_frame_summary"""
    _fields_ = [('n_used', C.c_longlong), ('n_nonfinite', C.c_longlong), ('mass', C.c_double), ('com', C.c_double * 3),
                ('momentum', C.c_double * 3), ('kinetic', C.c_double), ('v_max', C.c_double), ('courant', C.c_double),
                ('lo', C.c_double * 3), ('hi', C.c_double * 3), ('J_min', C.c_double), ('J_max', C.c_double)]


FE_SUMMARY_MAX_GROUPS = 32


class FeLossSel(C.Structure):
    """include/fluidengine_ext.h: the particles a loss term runs over"""
    _fields_ = [('pid_lo', C.c_int), ('pid_hi', C.c_int), ('mat', C.c_int), ('require_used', C.c_int)]


class FeLossTerm(C.Structure):
    """include/fluidengine_ext.h: one term of a loss-term program (fe_task_loss_set_terms)"""
    _fields_ = [('kind', C.c_int), ('axis_mask', C.c_int), ('a', FeLossSel), ('b', FeLossSel), ('c', C.c_double * 3), ('weight', C.c_double)]


FE_TASK_LOSS_MAX_TERMS = 8
FE_TASK_LOSS_MAX_PAIR_TERMS = 2
FE_TASK_LOSS_MAX_DENSITY_TERMS = 2
FE_TASK_LOSS_MAX_NEAREST_TERMS = 2
FE_TERM_L1_CONST, FE_TERM_SQ_CONST, FE_TERM_L1_REF, FE_TERM_PAIR_L1, FE_TERM_DENSITY_SQ = 0, 1, 2, 3, 4
FE_TERM_NEAREST_SQ, FE_TERM_COVER_SQ = 5, 6
FE_CLOUD_MAX = 4
FE_CLOUD_MAX_POINTS = 1 << 20
FE_CLOUD_COORD_MAX = 2.0


class FeDensitySpec(C.Structure):
    """include/fluidengine_ext.h: a density field -- n cells per axis (1 = projected) of size `cell` from the corner `origin`"""
    _fields_ = [('origin', C.c_double * 3), ('cell', C.c_double * 3), ('n', C.c_int * 3), ('pad', C.c_int)]


FE_DENSITY_MAX_FIELDS = 2
FE_DENSITY_MAX_CELLS = 1 << 21
FE_DENSITY_LDS_CELLS = 8192
FE_FIELD_OBS_MAX = 4


class FeSmokeSummary(C.Structure):
    """include/fluidengine_ext.h: the record of fe_smoke_summary"""
    _fields_ = [('n_cells', C.c_longlong), ('n_nonfinite', C.c_longlong), ('v_max', C.c_double), ('courant', C.c_double),
                ('kinetic', C.c_double), ('q_sum', C.c_double * 3), ('q_min', C.c_double * 3), ('q_max', C.c_double * 3)]


FE_SMOKE_MAX_LISTS = 4
FE_SMOKE_MAX_LIST_CELLS = 1 << 16
FE_SMOKE_L1, FE_SMOKE_SQ = 0, 1

FE_RENDER_MAX_LIGHTS = 4
FE_RENDER_MAX_SETS = 2
FE_RENDER_MAX_POINTS = 1 << 20
FE_RENDER_MAX_SIZE = 4096
FE_RENDER_LANE_PIXELS = 25


class FeRenderCamera(C.Structure):
    """include/fluidengine_ext.h: the camera of fe_render_setup -- position, an orthonormal basis, focal length in pixels"""
    _fields_ = [('pos', C.c_double * 3), ('right', C.c_double * 3), ('up', C.c_double * 3), ('fwd', C.c_double * 3),
                ('focal', C.c_double), ('near', C.c_double), ('max_radius_px', C.c_double), ('width', C.c_int), ('height', C.c_int)]


class FeRenderLights(C.Structure):
    """include/fluidengine_ext.h: ambient and background colour and up to FE_RENDER_MAX_LIGHTS point lights"""
    _fields_ = [('ambient', C.c_double * 3), ('background', C.c_double * 3), ('pos', (C.c_double * 3) * FE_RENDER_MAX_LIGHTS),
                ('color', (C.c_double * 3) * FE_RENDER_MAX_LIGHTS), ('n_lights', C.c_int), ('pad', C.c_int)]


FE_RENDER_MAX_VOLUMES = 16
FE_RENDER_MAX_MARCH = 4096
FE_RENDER_VOL_NONE, FE_RENDER_VOL_STATIC, FE_RENDER_VOL_EFFECTOR, FE_RENDER_VOL_OWN = 0, 1, 2, 3


class FeRenderScene(C.Structure):
    """include/fluidengine_ext.h: the scene of fe_render_set_scene -- the march of the volumes and the smoke field's slab, radius and colours"""
    _fields_ = [('march_step', C.c_double), ('smoke_radius', C.c_double), ('cold', C.c_double * 3), ('hot', C.c_double * 3),
                ('bisect_iters', C.c_int), ('draw_smoke', C.c_int), ('lo', C.c_int), ('hi', C.c_int)]


class FeSurfaceParams(C.Structure):
    """include/fluidengine_ext.h: the parameters of fe_surface_set -- how the liquid layer is drawn, smoothed, lit and blended"""
    _fields_ = [('radius_scale', C.c_double), ('range', C.c_double), ('absorb', C.c_double), ('alpha_min', C.c_double), ('specular', C.c_double),
                ('smooth_iters', C.c_int), ('smooth_radius_px', C.c_int), ('shininess_log2', C.c_int), ('pad', C.c_int)]


class FeContactRecord(C.Structure):
    """include/fluidengine_ext.h: what one collider's contact law gave to the material in one substep (fe_contact_wrench)"""
    _fields_ = [('impulse', C.c_double * 3), ('ang_impulse', C.c_double * 3), ('ref', C.c_double * 3), ('n_particles', C.c_longlong),
                ('n_nodes', C.c_longlong), ('valid', C.c_int), ('kind', C.c_int)]


# the same record as a numpy structured dtype: Engine.contact_wrench returns an array [n, n_records] of it
CONTACT_DTYPE = np.dtype([('impulse', np.float64, 3), ('ang_impulse', np.float64, 3), ('ref', np.float64, 3), ('n_particles', np.int64),
                          ('n_nodes', np.int64), ('valid', np.int32), ('kind', np.int32)])


# every symbol include/fluidengine.h declares (tests assert the libraries export all of them)
ABI_SYMBOLS = [
    'fe_create', 'fe_destroy', 'fe_last_error', 'fe_backend', 'fe_real_size', 'fe_sync',
    'fe_set_option', 'fe_get_option', 'fe_init_particles', 'fe_substep', 'fe_substep_grad', 'fe_step',
    'fe_step_grad', 'fe_step_batch', 'fe_step_grad_batch', 'fe_get_frame', 'fe_set_frame', 'fe_get_frame_dev', 'fe_set_frame_dev', 'fe_copy_frame', 'fe_copy_grad',
    'fe_reset_grad', 'fe_reset_grad_till_frame', 'fe_get_grad', 'fe_add_grad', 'fe_get_mat',
    'fe_add_static', 'fe_eff_set_mesh', 'fe_add_effector', 'fe_eff_set_act_range', 'fe_eff_get_state', 'fe_eff_set_state',
    'fe_eff_get_vw', 'fe_eff_set_vw', 'fe_eff_get_sr', 'fe_eff_set_sr', 'fe_eff_set_action', 'fe_eff_set_action_grad',
    'fe_eff_apply_action_p', 'fe_eff_apply_action_p_grad', 'fe_eff_get_action_grad',
    'fe_agent_copy_frame', 'fe_agent_copy_grad', 'fe_agent_reset_grad_till_frame', 'fe_agent_set_collector', 'fe_mesh_sdf', 'fe_add_grad_dev', 'fe_loss_alloc', 'fe_loss_set_target',
    'fe_loss_clear', 'fe_loss_step', 'fe_loss_step_grad', 'fe_loss_get', 'fe_get_stats', 'fe_get_work_stats', 'fe_get_work_stats_n',
    'fe_smoke_create', 'fe_smoke_step', 'fe_smoke_step_grad', 'fe_smoke_get_frame', 'fe_smoke_set_frame', 'fe_smoke_get_grad',
    'fe_smoke_add_grad', 'fe_smoke_copy_frame', 'fe_smoke_copy_grad', 'fe_smoke_reset_grad', 'fe_smoke_reset_grad_till_frame',
    'fe_timer_start', 'fe_timer_stop_ms', 'fe_profile_enable', 'fe_profile_read',
]

# include/fluidengine_ext.h: HIP-engine extensions.  Looked up on the HIP library only -- the oracle libraries do not have them, and
# missing_symbols() keeps asking for ABI_SYMBOLS alone.
EXT_SYMBOLS = ['fe_param_grad_get', 'fe_param_grad_get_dev', 'fe_param_grad_reset',
               'fe_obs_set_particles', 'fe_obs_get', 'fe_obs_get_dev', 'fe_summary_set_groups', 'fe_frame_summary',
               'fe_task_loss_alloc', 'fe_task_loss_set_terms', 'fe_task_loss_set_ref', 'fe_task_loss_clear', 'fe_task_loss_step',
               'fe_task_loss_step_grad', 'fe_task_loss_get',
               'fe_density_set_field', 'fe_density_set_target', 'fe_density_get',
               'fe_cloud_set', 'fe_cloud_query',
               'fe_smoke_cells_set', 'fe_smoke_cells_get', 'fe_smoke_cells_get_dev', 'fe_smoke_loss_alloc', 'fe_smoke_loss_set',
               'fe_smoke_loss_clear', 'fe_smoke_loss_step', 'fe_smoke_loss_step_grad', 'fe_smoke_loss_get', 'fe_smoke_summary',
               'fe_render_setup', 'fe_render_set_colors', 'fe_render_set_points', 'fe_render_frame', 'fe_render_get', 'fe_render_get_dev',
               'fe_render_set_volume', 'fe_render_set_scene', 'fe_render_scene_frame',
               'fe_contact_count', 'fe_contact_wrench',
               'fe_obs_add_grad', 'fe_obs_add_grad_dev', 'fe_eff_add_state_grad', 'fe_eff_add_state_grad_dev', 'fe_eff_get_state_grad',
               'fe_eff_get_state_dev', 'fe_eff_set_action_dev', 'fe_eff_get_action_grad_dev',
               'fe_smoke_cells_add_grad', 'fe_smoke_cells_add_grad_dev',
               'fe_smoke_obs_get', 'fe_smoke_obs_get_dev', 'fe_smoke_obs_add_grad', 'fe_smoke_obs_add_grad_dev',
               'fe_eff_add_sr_grad', 'fe_eff_get_sr_grad',
               'fe_field_obs_set', 'fe_field_obs_get', 'fe_field_obs_get_dev', 'fe_field_obs_add_grad', 'fe_field_obs_add_grad_dev',
               'fe_surface_set', 'fe_surface_frame', 'fe_surface_get', 'fe_surface_get_dev']


class EngineLib:
    """One loaded shared library exporting the FluidEngine ABI."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise FeEngineError(f'FluidEngine library not found: {path}')
        self.path = path
        if os.path.basename(path).endswith('_hip.so'):
            # torch wheels bundle their own libamdhip64; whichever HIP runtime is mapped first serves the whole process,
            # and torch sees no GPU when /opt/rocm's was mapped first.  The host layer shares device memory with torch
            # (ckpt_dest='gpu', the action-gradient all-reduce), so let torch map its runtime before the engine binds it.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        self.lib = C.CDLL(path)
        lib = self.lib
        lib.fe_real_size.restype = C.c_int
        lib.fe_backend.restype = C.c_char_p
        self.real_size = lib.fe_real_size()
        self.backend = lib.fe_backend().decode()
        self.real = C.c_float if self.real_size == 4 else C.c_double
        self.dtype = np.float32 if self.real_size == 4 else np.float64
        self.FeBoundary, self.FeConfig, self.FeEffectorDesc, self.FeSdfDesc, self.FeSmokeConfig = _structs(self.real)
        lib.fe_create.restype = C.c_void_p
        lib.fe_create.argtypes = [C.c_void_p]
        lib.fe_destroy.restype = None
        lib.fe_destroy.argtypes = [C.c_void_p]
        lib.fe_last_error.restype = C.c_char_p
        lib.fe_last_error.argtypes = [C.c_void_p]
        lib.fe_timer_stop_ms.restype = C.c_double
        lib.fe_timer_stop_ms.argtypes = [C.c_void_p]
        lib.fe_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        if hasattr(lib, 'fe_get_option'):                 # (A/B builds of earlier rounds, scripts/ab_phases.py `lib=`, do not have it)
            lib.fe_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]

    def mesh_sdf(self, verts, faces, points, device=0):
        """fe_mesh_sdf: signed distance of points[M,3] to the triangle mesh (verts[nv,3], faces[nf,3]); float32 out."""
        v = np.ascontiguousarray(verts, np.float32); f = np.ascontiguousarray(faces, np.int32); p = np.ascontiguousarray(points, np.float32)
        assert v.ndim == 2 and v.shape[1] == 3 and f.ndim == 2 and f.shape[1] == 3 and p.ndim == 2 and p.shape[1] == 3
        out = np.empty((len(p),), np.float32)
        rc = self.lib.fe_mesh_sdf(int(device), v.ctypes.data_as(C.c_void_p), len(v), f.ctypes.data_as(C.c_void_p), len(f),
                                  p.ctypes.data_as(C.c_void_p), C.c_longlong(len(p)), out.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise FeEngineError(self.lib.fe_last_error(None).decode())
        return out

    def missing_symbols(self):
        return [s for s in ABI_SYMBOLS if not hasattr(self.lib, s)]

    def missing_ext_symbols(self):
        return [s for s in EXT_SYMBOLS if not hasattr(self.lib, s)]

    @property
    def has_ext(self):
        """the library exports include/fluidengine_ext.h (the HIP engine does, the oracle libraries do not)"""
        return not self.missing_ext_symbols()

    def make_boundary(self, type='cube', lower=(0.05, 0.05, 0.05), upper=(0.95, 0.95, 0.95),
                      y_range=(0.05, 0.95), xz_center=(0.5, 0.5), xz_radius=0.45,
                      restitution=0.0, lock_dims=()):
        """boundaries.py:136-141 create_boundary(), as the ABI struct."""
        b = self.FeBoundary()
        if type == 'cube':
            b.type = FE_BOUNDARY_CUBE
            lo = np.asarray(lower, dtype=self.dtype)
            up = np.asarray(upper, dtype=self.dtype)
            assert (up >= lo).all()
            b.lower[:] = [float(t) for t in lo]
            b.upper[:] = [float(t) for t in up]
        elif type == 'cylinder':
            b.type = FE_BOUNDARY_CYLINDER
            yr = np.asarray(y_range, dtype=self.dtype)
            b.lower[:] = [0.0, float(yr[0]), 0.0]
            b.upper[:] = [1.0, float(yr[1]), 1.0]
            c = np.asarray(xz_center, dtype=self.dtype)
            b.xz_center[:] = [float(c[0]), float(c[1])]
            b.xz_radius = float(xz_radius)
        else:
            raise AssertionError(f'unknown boundary type {type}')
        b.restitution = float(restitution)
        b.lock_dims = sum(1 << int(d) for d in lock_dims)
        return b


_hip_lib = None


def load_hip():
    """The product library.  Fails loudly when the HIP extension is not built."""
    global _hip_lib
    if _hip_lib is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise FeEngineError(
                f'{HIP_LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                '(hipcc --offload-arch=gfx950).  There is no CPU fallback.')
        _hip_lib = EngineLib(HIP_LIB_PATH)
    return _hip_lib


class Engine:
    """Thin object wrapper over one FeEngine handle.  All arrays are numpy, C-contiguous,
    in the library's real dtype; integer arrays are int32."""

    def __init__(self, elib, *, n_grid, n_particles, max_substeps_local, n_substeps,
                 max_action_steps, dt, p_vol, gravity, boundary, device=0):
        self.elib = elib
        self.lib = elib.lib
        self.dtype = elib.dtype
        cfg = elib.FeConfig()
        cfg.struct_size = C.sizeof(elib.FeConfig)
        cfg.n_grid = int(n_grid)
        cfg.n_particles = int(n_particles)
        cfg.max_substeps_local = int(max_substeps_local)
        cfg.n_substeps = int(n_substeps)
        cfg.max_action_steps = int(max_action_steps)
        cfg.dt = float(dt)
        cfg.p_vol = float(p_vol)
        cfg.gravity[:] = [float(g) for g in gravity]
        cfg.boundary = boundary
        cfg.device = int(device)
        self.device = int(device)
        self.cfg = cfg
        self.N = int(n_particles)
        self.n_obs = 0                                       # length of the observation list (obs_set_particles)
        self.n_summary_groups = 0                            # groups of the frame summary (summary_set_groups)
        self._cloud_n = {}                                   # cloud id -> number of points (cloud_set)
        self._density_n = {}                                 # field id -> cells per axis (density_set_field)
        self._field_obs_n = {}                               # observation field id -> (channels, n0, n1, n2) (field_obs_set)
        self.n_task_terms = 0                                # terms of the loss-term program (task_loss_set_terms)
        self._smoke_list_n = {}                              # list id -> length of the smoke cell list (smoke_cells_set)
        self._eff_action_dim = {}                            # effector index -> action_dim (add_effector): shapes of the device-pointer calls
        self.h = self.lib.fe_create(C.byref(cfg))
        if not self.h:
            raise FeEngineError('fe_create failed: ' + self.lib.fe_last_error(None).decode())
        self.h = C.c_void_p(self.h)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.fe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers
    def _ck(self, rc):
        if rc != 0:
            raise FeEngineError(self.lib.fe_last_error(self.h).decode())

    def _r(self, a, shape=None):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if shape is not None:
            assert a.shape == tuple(shape), f'expected shape {shape}, got {a.shape}'
        return a, a.ctypes.data_as(C.c_void_p)

    def _i(self, a, shape=None):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=np.int32)
        if shape is not None:
            assert a.shape == tuple(shape), f'expected shape {shape}, got {a.shape}'
        return a, a.ctypes.data_as(C.c_void_p)

    def _out(self, a, shape, dtype=None):
        """Validate a caller-provided output array (must be writable in place)."""
        dtype = dtype or self.dtype
        assert isinstance(a, np.ndarray) and a.dtype == dtype and a.flags['C_CONTIGUOUS'] and a.shape == tuple(shape)
        return a.ctypes.data_as(C.c_void_p)

    # ---- lifecycle
    def sync(self):
        self._ck(self.lib.fe_sync(self.h))

    def set_option(self, name, value):
        self._ck(self.lib.fe_set_option(self.h, name.encode(), float(value)))

    OPTION_NAMES = ('sort_interval', 'item_max', 'grid_store', 'p2g_grad_waves', 'g2p_grad_v', 'loose_max', 'xcd_map', 'write_through',
                    'wave_sort', 'lane_split', 'fold_reorder', 'compact_F', 'fuse_g2p', 'fuse_bwd', 'quad_min_units', 'pgg_quad_min_units', 'quad_max', 'quad_fit', 'pack_units', 'wgrid_cap', 'wgrid_cap_g2p', 'wgrid_cap_pgg', 'ggrid_cap', 'grid_list_launch', 'grid_hint', 'grid_hint_margin', 'grid_one_cap', 'collide_type')

    def get_option(self, name):
        v = C.c_double(0.0)
        self._ck(self.lib.fe_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def get_options(self):
        """every tunable as the engine holds it now: defaults, fe_set_option calls and FE_* environment variables alike"""
        return {n: self.get_option(n) for n in self.OPTION_NAMES}

    def init_particles(self, x, used, mat, mat_cls, mu, lam, rho, body_id):
        N = self.N
        k0, x_ = self._r(x, (N, 3)); k1, u_ = self._i(used, (N,)); k2, m_ = self._i(mat, (N,))
        k3, c_ = self._i(mat_cls, (N,)); k4, mu_ = self._r(mu, (N,)); k5, la_ = self._r(lam, (N,))
        k6, rh_ = self._r(rho, (N,)); k7, b_ = self._i(body_id, (N,))
        self._ck(self.lib.fe_init_particles(self.h, x_, u_, m_, c_, mu_, la_, rh_, b_))

    # ---- hot path
    def substep(self, f, f_global, act):
        self._ck(self.lib.fe_substep(self.h, int(f), int(f_global), int(bool(act))))

    def substep_grad(self, f, f_global, act):
        self._ck(self.lib.fe_substep_grad(self.h, int(f), int(f_global), int(bool(act))))

    def step(self, f0, f_global0, n, act):
        self._ck(self.lib.fe_step(self.h, int(f0), int(f_global0), int(n), int(bool(act))))

    def step_grad(self, f0, f_global0, n, act):
        self._ck(self.lib.fe_step_grad(self.h, int(f0), int(f_global0), int(n), int(bool(act))))

    # ---- state I/O
    def get_frame(self, f, x=None, v=None, C_=None, F=None, used=None):
        """Fill the given arrays in place (like readframe, mpm:555-564); None = skip."""
        N = self.N
        px = self._out(x, (N, 3)) if x is not None else None
        pv = self._out(v, (N, 3)) if v is not None else None
        pC = self._out(C_, (N, 3, 3)) if C_ is not None else None
        pF = self._out(F, (N, 3, 3)) if F is not None else None
        pu = self._out(used, (N,), np.int32) if used is not None else None
        self._ck(self.lib.fe_get_frame(self.h, int(f), px, pv, pC, pF, pu))

    def set_frame(self, f, x=None, v=None, C_=None, F=None, used=None):
        N = self.N
        k0, px = self._r(x, (N, 3)); k1, pv = self._r(v, (N, 3)); k2, pC = self._r(C_, (N, 3, 3))
        k3, pF = self._r(F, (N, 3, 3)); k4, pu = self._i(used, (N,))
        self._ck(self.lib.fe_set_frame(self.h, int(f), px, pv, pC, pF, pu))

    @staticmethod
    def _handles(engines):
        arr = (C.c_void_p * len(engines))(*[e.h for e in engines])
        return arr

    @staticmethod
    def step_batch(engines, f0, f_global0, n, act):
        """fe_step_batch: the same n substeps for every engine of the list (lockstep environments, one launch per phase)"""
        e0 = engines[0]
        e0._ck(e0.lib.fe_step_batch(Engine._handles(engines), len(engines), int(f0), int(f_global0), int(n), int(bool(act))))

    @staticmethod
    def step_grad_batch(engines, f0, f_global0, n, act):
        e0 = engines[0]
        e0._ck(e0.lib.fe_step_grad_batch(Engine._handles(engines), len(engines), int(f0), int(f_global0), int(n), int(bool(act))))

    def copy_frame(self, src, dst):
        self._ck(self.lib.fe_copy_frame(self.h, int(src), int(dst)))

    def copy_grad(self, src, dst):
        self._ck(self.lib.fe_copy_grad(self.h, int(src), int(dst)))

    def reset_grad(self):
        self._ck(self.lib.fe_reset_grad(self.h))

    def reset_grad_till_frame(self, f):
        self._ck(self.lib.fe_reset_grad_till_frame(self.h, int(f)))

    def get_grad(self, f):
        N = self.N
        gx = np.zeros((N, 3), self.dtype); gv = np.zeros((N, 3), self.dtype)
        gC = np.zeros((N, 3, 3), self.dtype); gF = np.zeros((N, 3, 3), self.dtype)
        self._ck(self.lib.fe_get_grad(self.h, int(f), gx.ctypes.data_as(C.c_void_p), gv.ctypes.data_as(C.c_void_p),
                                      gC.ctypes.data_as(C.c_void_p), gF.ctypes.data_as(C.c_void_p)))
        return gx, gv, gC, gF

    # ---- state that stays on the device: torch tensors on the engine's GPU (the reference's readframe/setframe accept them)
    @staticmethod
    def _tptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _torch_fence(self, *tensors):
        """The engine's stream is non-blocking: nothing orders it with torch's streams.  Before the engine reads or overwrites a
        torch tensor, whatever torch has queued on it -- the fill of a fresh allocation, an earlier read of a staging tensor,
        a producer on a side stream -- has to be finished: every stream of the tensors' devices is drained (the engine calls
        themselves return after the engine's stream has drained)."""
        done = set()
        for t in tensors:
            if t is not None and t.device not in done:
                import torch
                torch.cuda.synchronize(t.device)
                done.add(t.device)

    def get_frame_dev(self, f, x=None, v=None, C_=None, F=None, used=None):
        self._torch_fence(x, v, C_, F, used)
        self._ck(self.lib.fe_get_frame_dev(self.h, int(f), self._tptr(x), self._tptr(v), self._tptr(C_), self._tptr(F), self._tptr(used)))

    def set_frame_dev(self, f, x=None, v=None, C_=None, F=None, used=None):
        self._torch_fence(x, v, C_, F, used)
        self._ck(self.lib.fe_set_frame_dev(self.h, int(f), self._tptr(x), self._tptr(v), self._tptr(C_), self._tptr(F), self._tptr(used)))

    def add_grad_dev(self, f, gx=None, gv=None, gC=None, gF=None):
        """fe_add_grad_dev: torch tensors on the engine's GPU (their device is synchronised here, whichever stream produced them)"""
        self._torch_fence(gx, gv, gC, gF)
        self._ck(self.lib.fe_add_grad_dev(self.h, int(f), self._tptr(gx), self._tptr(gv), self._tptr(gC), self._tptr(gF)))

    def add_grad(self, f, gx=None, gv=None, gC=None, gF=None):
        N = self.N
        k0, px = self._r(gx, (N, 3)); k1, pv = self._r(gv, (N, 3)); k2, pC = self._r(gC, (N, 3, 3)); k3, pF = self._r(gF, (N, 3, 3))
        self._ck(self.lib.fe_add_grad(self.h, int(f), px, pv, pC, pF))

    def get_mat(self):
        m = np.zeros((self.N,), np.int32)
        self._ck(self.lib.fe_get_mat(self.h, m.ctypes.data_as(C.c_void_p)))
        return m

    # ---- material-parameter gradients (include/fluidengine_ext.h; HIP engine only, no fallback)
    def _need_ext(self, what='material-parameter gradients'):
        if not self.elib.has_ext:
            raise FeEngineError(f'{what} are not available on {self.elib.backend}')

    def param_grad_enable(self, on=True):
        """fe_set_option('param_grad'): every backward substep from here on adds d loss / d (mu, lam, rho) of its particles to the accumulators"""
        self._need_ext()
        self.set_option('param_grad', 1 if on else 0)

    def get_param_grad(self):
        """{'mu', 'lam', 'rho'}: fp64 arrays [N] in particle order, what the backward substeps since the last reset_grad() added up"""
        self._need_ext()
        out = {k: np.zeros((self.N,), np.float64) for k in ('mu', 'lam', 'rho')}
        self._ck(self.lib.fe_param_grad_get(self.h, *[out[k].ctypes.data_as(C.c_void_p) for k in ('mu', 'lam', 'rho')]))
        return out

    def get_param_grad_dev(self, mu=None, lam=None, rho=None):
        """the same into float64 torch tensors [N] on the engine's GPU (None = skip)"""
        self._need_ext()
        self._torch_fence(mu, lam, rho)
        self._ck(self.lib.fe_param_grad_get_dev(self.h, self._tptr(mu), self._tptr(lam), self._tptr(rho)))

    def reset_param_grad(self):
        self._need_ext()
        self._ck(self.lib.fe_param_grad_reset(self.h))

    # ---- frame reads that stay on the GPU (include/fluidengine_ext.h; HIP engine only, no fallback)
    def obs_set_particles(self, ids):
        """fe_obs_set_particles: the particle ids get_obs / get_obs_dev return rows for (duplicates allowed; None or empty removes the list)"""
        self._need_ext('device observations')
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        n = 0 if ids is None else int(ids.size)
        self._ck(self.lib.fe_obs_set_particles(self.h, ids.ctypes.data_as(C.c_void_p) if n else None, n))
        self.n_obs = n

    def get_obs(self, f):
        """{'x' [n,3], 'v' [n,3], 'used' [n]}: the listed particles' rows of frame f -- n rows are copied to the host, not N"""
        self._need_ext('device observations')
        n = self.n_obs
        out = {'x': np.zeros((n, 3), self.dtype), 'v': np.zeros((n, 3), self.dtype), 'used': np.zeros((n,), np.int32)}
        self._ck(self.lib.fe_obs_get(self.h, int(f), *[out[k].ctypes.data_as(C.c_void_p) for k in ('x', 'v', 'used')]))
        return out

    def get_obs_dev(self, f, x=None, v=None, used=None):
        """the same into torch tensors on the engine's GPU (x, v: engine dtype [n,3]; used: int32 [n]; None = skip)"""
        self._need_ext('device observations')
        import torch
        n = self.n_obs
        for name, t, shape, dt in (('x', x, (n, 3), torch.float32), ('v', v, (n, 3), torch.float32), ('used', used, (n,), torch.int32)):
            if t is None:
                continue
            if not (t.is_cuda and t.device.index == self.device and tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous()):
                raise FeEngineError(f'get_obs_dev: {name} must be a contiguous {dt} tensor of shape {shape} on cuda:{self.device}, '
                                    f'got {t.dtype} {tuple(t.shape)} on {t.device}')
        self._torch_fence(x, v, used)
        self._ck(self.lib.fe_obs_get_dev(self.h, int(f), self._tptr(x), self._tptr(v), self._tptr(used)))

    def summary_set_groups(self, group, n_groups=0):
        """fe_summary_set_groups: group[N] by particle id, values in [-1, n_groups) (-1: in no group); None removes the groups"""
        self._need_ext('frame summaries')
        if group is None:
            self._ck(self.lib.fe_summary_set_groups(self.h, None, 0))
            self.n_summary_groups = 0
            return
        k, p = self._i(group, (self.N,))
        self._ck(self.lib.fe_summary_set_groups(self.h, p, int(n_groups)))
        self.n_summary_groups = int(n_groups)

    def frame_summary(self, f):
        """fe_frame_summary: a list of dicts, one per group, the whole-frame record last (fields of FeFrameSummary; vectors as fp64 arrays)"""
        self._need_ext('frame summaries')
        n = self.n_summary_groups + 1
        rec = (FeFrameSummary * n)()
        self._ck(self.lib.fe_frame_summary(self.h, int(f), C.byref(rec), n, C.sizeof(FeFrameSummary)))
        return [{k: (np.array(getattr(r, k), np.float64) if k in ('com', 'momentum', 'lo', 'hi') else getattr(r, k)) for k, _ in FeFrameSummary._fields_}
                for r in rec]

    # ---- closed-loop policies: observation and tool-state adjoints, device forms of the per-step crossings
    #      (include/fluidengine_ext.h; HIP engine only, no fallback)
    _POLICY_IO = 'closed-loop policy calls'

    def _dev_tensor(self, call, name, t, shape):
        """a contiguous tensor of the engine's dtype and the given shape on the engine's GPU, or FeEngineError (None passes)"""
        if t is None:
            return
        import torch
        if not (t.is_cuda and t.device.index == self.device and tuple(t.shape) == tuple(shape) and t.dtype == torch.float32 and t.is_contiguous()):
            raise FeEngineError(f'{call}: {name} must be a contiguous torch.float32 tensor of shape {tuple(shape)} on cuda:{self.device}, '
                                f'got {t.dtype} {tuple(t.shape)} on {t.device}')

    def obs_add_grad(self, f, gx=None, gv=None):
        """fe_obs_add_grad: row i of gx / gv [n,3] is added to the x / v adjoint of particle ids[i] (obs_set_particles) of frame f; rows of a
        particle listed several times are summed in list order in fp32 first.  n rows cross PCIe, not N; F's adjoint is not touched."""
        self._need_ext(self._POLICY_IO)
        n = self.n_obs
        k0, px = self._r(gx, (n, 3)); k1, pv = self._r(gv, (n, 3))
        self._ck(self.lib.fe_obs_add_grad(self.h, int(f), px, pv))

    def obs_add_grad_dev(self, f, gx=None, gv=None):
        """the same from torch tensors on the engine's GPU (engine dtype [n,3]; None = skip)"""
        self._need_ext(self._POLICY_IO)
        n = self.n_obs
        self._dev_tensor('obs_add_grad_dev', 'gx', gx, (n, 3)); self._dev_tensor('obs_add_grad_dev', 'gv', gv, (n, 3))
        self._torch_fence(gx, gv)
        self._ck(self.lib.fe_obs_add_grad_dev(self.h, int(f), self._tptr(gx), self._tptr(gv)))

    def eff_add_state_grad(self, e, f, g7):
        """fe_eff_add_state_grad: gpos[f] += g7[:3], gquat[f] += g7[3:7] of effector e"""
        self._need_ext(self._POLICY_IO)
        k, p = self._r(g7, (7,))
        self._ck(self.lib.fe_eff_add_state_grad(self.h, int(e), int(f), p))

    def eff_add_state_grad_dev(self, e, f, g7):
        """the same from a torch tensor [7] on the engine's GPU"""
        self._need_ext(self._POLICY_IO)
        if g7 is None:
            raise FeEngineError('eff_add_state_grad_dev: g7 is None')
        self._dev_tensor('eff_add_state_grad_dev', 'g7', g7, (7,))
        self._torch_fence(g7)
        self._ck(self.lib.fe_eff_add_state_grad_dev(self.h, int(e), int(f), self._tptr(g7)))

    def eff_get_state_grad(self, e, f):
        """fe_eff_get_state_grad: (gpos[f], gquat[f]) of effector e as one array [7]"""
        self._need_ext(self._POLICY_IO)
        g = np.zeros((7,), self.dtype)
        self._ck(self.lib.fe_eff_get_state_grad(self.h, int(e), int(f), g.ctypes.data_as(C.c_void_p)))
        return g

    def eff_get_state_dev(self, e, f, s7):
        """fe_eff_get_state_dev: (pos[f], quat[f]) of effector e into a torch tensor [7] on the engine's GPU"""
        self._need_ext(self._POLICY_IO)
        if s7 is None:
            raise FeEngineError('eff_get_state_dev: s7 is None')
        self._dev_tensor('eff_get_state_dev', 's7', s7, (7,))
        self._torch_fence(s7)
        self._ck(self.lib.fe_eff_get_state_dev(self.h, int(e), int(f), self._tptr(s7)))

    def eff_set_action_dev(self, e, s, s_global, n_substeps, action):
        """fe_eff_set_action_dev: eff_set_action with the action a torch tensor [action_dim] on the engine's GPU"""
        self._need_ext(self._POLICY_IO)
        if action is None:
            raise FeEngineError('eff_set_action_dev: action is None')
        self._dev_tensor('eff_set_action_dev', 'action', action, (self._eff_action_dim.get(int(e), 0),))
        self._torch_fence(action)
        self._ck(self.lib.fe_eff_set_action_dev(self.h, int(e), int(s), int(s_global), int(n_substeps), self._tptr(action)))

    def eff_get_action_grad_dev(self, e, s, n, out):
        """fe_eff_get_action_grad_dev: gabuf[s:s+n] of effector e into a torch tensor [n, action_dim] on the engine's GPU"""
        self._need_ext(self._POLICY_IO)
        if out is None:
            raise FeEngineError('eff_get_action_grad_dev: out is None')
        self._dev_tensor('eff_get_action_grad_dev', 'out', out, (int(n), self._eff_action_dim.get(int(e), 0)))
        self._torch_fence(out)
        self._ck(self.lib.fe_eff_get_action_grad_dev(self.h, int(e), int(s), int(n), self._tptr(out)))

    # ---- contact wrenches (include/fluidengine_ext.h; HIP engine only, no fallback)
    def contact_count(self):
        """fe_contact_count: the records fe_contact_wrench writes per substep -- the effectors, then the statics"""
        self._need_ext('contact wrenches')
        return int(self.lib.fe_contact_count(self.h))

    def contact_wrench(self, f0, n=1):
        """fe_contact_wrench: a structured array [n, n_records] (CONTACT_DTYPE) -- per substep f0 .. f0 + n - 1 and collider the linear and
        angular impulse its contact law gave to the material; valid == 0 where the frame's grid is not in the store"""
        self._need_ext('contact wrenches')
        n_rec = self.contact_count()
        out = np.zeros((int(n), n_rec), CONTACT_DTYPE)
        assert CONTACT_DTYPE.itemsize == C.sizeof(FeContactRecord)
        # (an engine without colliders: the call still checks its arguments and writes nothing)
        buf = out if n_rec else np.zeros((1,), CONTACT_DTYPE)
        self._ck(self.lib.fe_contact_wrench(self.h, int(f0), int(n), buf.ctypes.data_as(C.c_void_p), max(n_rec, 1), C.sizeof(FeContactRecord)))
        return out

    # ---- task losses as loss-term programs (include/fluidengine_ext.h; HIP engine only, no fallback)
    def task_loss_alloc(self, max_loss_steps):
        """fe_task_loss_alloc: step_loss[max_loss_steps] and the per-term values, fp64 on the device, zeroed"""
        self._need_ext('device task losses')
        self._ck(self.lib.fe_task_loss_alloc(self.h, int(max_loss_steps)))

    def task_loss_set_terms(self, terms):
        """fe_task_loss_set_terms: a sequence of FeLossTerm, or of objects with to_c() (losses/term_program.py); None or empty removes the program"""
        self._need_ext('device task losses')
        terms = [t if isinstance(t, FeLossTerm) else t.to_c() for t in (terms or [])]
        arr = (FeLossTerm * max(1, len(terms)))(*terms)
        self._ck(self.lib.fe_task_loss_set_terms(self.h, C.byref(arr), len(terms), C.sizeof(FeLossTerm)))
        self.n_task_terms = len(terms)

    def task_loss_set_ref(self, f):
        """fe_task_loss_set_ref: FE_TERM_L1_REF measures against the positions of frame f from here on (copied on the device)"""
        self._need_ext('device task losses')
        self._ck(self.lib.fe_task_loss_set_ref(self.h, int(f)))

    def task_loss_clear(self):
        self._need_ext('device task losses')
        self._ck(self.lib.fe_task_loss_clear(self.h))

    def task_loss_step(self, s, f):
        """fe_task_loss_step: step_loss[s] += the program's value on frame f (enqueued; does not wait)"""
        self._need_ext('device task losses')
        self._ck(self.lib.fe_task_loss_step(self.h, int(s), int(f)))

    def task_loss_step_grad(self, s, f, scale=1.0):
        """fe_task_loss_step_grad: x.grad[f] += (float)(scale * d value / d x) (enqueued; does not wait)"""
        self._need_ext('device task losses')
        self._ck(self.lib.fe_task_loss_step_grad(self.h, int(s), int(f), C.c_double(float(scale))))

    def task_loss_get(self, n, s0=0, terms=False):
        """step_loss[s0:s0+n] as a fp64 array; with terms=True also the per-term values [n_terms, n].  Waits for the engine's stream."""
        self._need_ext('device task losses')
        sl = np.zeros((n,), np.float64)
        tl = np.zeros((self.n_task_terms, n), np.float64) if terms else None
        self._ck(self.lib.fe_task_loss_get(self.h, int(s0), int(n), sl.ctypes.data_as(C.c_void_p),
                                           tl.ctypes.data_as(C.c_void_p) if terms and tl.size else None))
        return (sl, tl) if terms else sl

    # ---- density fields (include/fluidengine_ext.h; HIP engine only, no fallback)
    def density_set_field(self, field, spec):
        """fe_density_set_field: spec is a FeDensitySpec or an object with to_c() (losses/term_program.DensityField); None removes the field.
        Setting a field drops its target."""
        self._need_ext('density fields')
        if spec is None:
            self._ck(self.lib.fe_density_set_field(self.h, int(field), None, C.sizeof(FeDensitySpec)))
            self._density_n.pop(int(field), None)
            return
        c = spec if isinstance(spec, FeDensitySpec) else spec.to_c()
        self._ck(self.lib.fe_density_set_field(self.h, int(field), C.byref(c), C.sizeof(FeDensitySpec)))
        self._density_n[int(field)] = tuple(int(v) for v in c.n)

    def density_set_target(self, field, target):
        """fe_density_set_target: the field's target, one value per cell (any shape with the field's cell count, C order), copied to the device"""
        self._need_ext('density fields')
        t = np.ascontiguousarray(target, np.float64).reshape(-1)
        self._ck(self.lib.fe_density_set_target(self.h, int(field), t.ctypes.data_as(C.c_void_p), C.c_longlong(t.size)))

    def density_field(self, f, field=0, sel=None):
        """fe_density_get: the density of frame f on the field, float64 shaped n, from the particles of sel (a FeLossSel or an object with
        to_c(); None: every used particle).  Waits for the engine's stream."""
        self._need_ext('density fields')
        n = self._density_n.get(int(field))
        if n is None:
            raise FeEngineError('density_field: the field is not set: density_set_field first')
        out = np.zeros(n, np.float64)
        c = None if sel is None else (sel if isinstance(sel, FeLossSel) else sel.to_c())
        self._ck(self.lib.fe_density_get(self.h, int(f), int(field), None if c is None else C.byref(c), out.ctypes.data_as(C.c_void_p), C.c_longlong(out.size)))
        return out

    # ---- field observations: density and momentum grids of a frame with their adjoints (include/fluidengine_ext.h; HIP engine only, no fallback)
    _FIELD_OBS = 'field observations'

    def field_obs_set(self, k, spec, sel=None, channels=4):
        """fe_field_obs_set: observation field k = the box spec (a FeDensitySpec or an object with to_c(); None removes the field), the particles
        of sel (a FeLossSel or an object with to_c(); None: every used particle) and 1 channel (density) or 4 (density, momentum x y z)"""
        self._need_ext(self._FIELD_OBS)
        if spec is None:
            self._ck(self.lib.fe_field_obs_set(self.h, int(k), None, C.sizeof(FeDensitySpec), None, int(channels)))
            self._field_obs_n.pop(int(k), None)
            return
        c = spec if isinstance(spec, FeDensitySpec) else spec.to_c()
        cs = None if sel is None else (sel if isinstance(sel, FeLossSel) else sel.to_c())
        self._ck(self.lib.fe_field_obs_set(self.h, int(k), C.byref(c), C.sizeof(FeDensitySpec), None if cs is None else C.byref(cs), int(channels)))
        self._field_obs_n[int(k)] = (int(channels),) + tuple(int(v) for v in c.n)

    def field_obs_shape(self, k):
        """(channels, n0, n1, n2) of observation field k"""
        n = self._field_obs_n.get(int(k))
        if n is None:
            raise FeEngineError('field_obs: the field is not set: field_obs_set first')
        return n

    def field_obs(self, f, k=0):
        """fe_field_obs_get: field k of frame f, float64 [channels, n0, n1, n2] on the host.  Waits for the engine's stream."""
        self._need_ext(self._FIELD_OBS)
        out = np.zeros(self.field_obs_shape(k), np.float64)
        self._ck(self.lib.fe_field_obs_get(self.h, int(f), int(k), out.ctypes.data_as(C.c_void_p), C.c_longlong(out.size)))
        return out

    def field_obs_dev(self, f, k=0, out=None):
        """fe_field_obs_get_dev: the same as a float32 torch tensor [channels, n0, n1, n2] on the engine's GPU (out: written in place); no
        frame and no field crosses to the host.  Returns the tensor."""
        self._need_ext(self._FIELD_OBS)
        shape = self.field_obs_shape(k)
        if out is None:
            import torch
            out = torch.empty(shape, dtype=torch.float32, device=f'cuda:{self.device}')
        self._dev_tensor('field_obs_dev', 'out', out, shape)
        self._torch_fence(out)
        self._ck(self.lib.fe_field_obs_get_dev(self.h, int(f), int(k), self._tptr(out)))
        return out

    def field_obs_add_grad(self, f, k, G):
        """fe_field_obs_add_grad: the cotangent G [channels, n0, n1, n2] of field k goes into the x and v adjoints of frame f.  A float32 torch
        tensor on the engine's GPU takes the _dev entry; anything else is staged from the host."""
        self._need_ext(self._FIELD_OBS)
        shape = self.field_obs_shape(k)
        if G is None:
            raise FeEngineError('field_obs_add_grad: G is None')
        if hasattr(G, 'data_ptr') and not isinstance(G, np.ndarray):
            self._dev_tensor('field_obs_add_grad', 'G', G, shape)
            self._torch_fence(G)
            self._ck(self.lib.fe_field_obs_add_grad_dev(self.h, int(f), int(k), self._tptr(G)))
            return
        keep, p = self._r(G, shape)
        self._ck(self.lib.fe_field_obs_add_grad(self.h, int(f), int(k), p))

    # ---- target clouds (include/fluidengine_ext.h; HIP engine only, no fallback)
    def cloud_set(self, cloud, xyz):
        """fe_cloud_set: the target cloud `cloud` = the points xyz [n, 3] (float32 words), copied to the device; None or empty removes it"""
        self._need_ext('target clouds')
        if xyz is None or len(xyz) == 0:
            self._ck(self.lib.fe_cloud_set(self.h, int(cloud), None, 0))
            self._cloud_n.pop(int(cloud), None)
            return
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self._ck(self.lib.fe_cloud_set(self.h, int(cloud), x.ctypes.data_as(C.c_void_p), int(len(x))))
        self._cloud_n[int(cloud)] = int(len(x))

    def cloud_query(self, f, cloud, sel=None, axis_mask=7):
        """fe_cloud_query: frame f against the cloud on the axes of axis_mask, for the particles of sel (a FeLossSel or an object with
        to_c(); None: every used particle).  Returns (nn_of_particle [N] int32 by pid, -1: not a query; d2_of_particle [N] float64;
        nn_of_point [n] int32 pid, -1: no particle; d2_of_point [n] float64).  Waits for the engine's stream."""
        self._need_ext('target clouds')
        n = self._cloud_n.get(int(cloud))
        if n is None:
            raise FeEngineError('cloud_query: the cloud is not set: cloud_set first')
        N = int(self.N)
        nn_p, d2_p = np.full((N,), -1, np.int32), np.zeros((N,), np.float64)
        nn_c, d2_c = np.full((n,), -1, np.int32), np.zeros((n,), np.float64)
        c = None if sel is None else (sel if isinstance(sel, FeLossSel) else sel.to_c())
        self._ck(self.lib.fe_cloud_query(self.h, int(f), int(cloud), None if c is None else C.byref(c), int(axis_mask),
                                         nn_p.ctypes.data_as(C.c_void_p), d2_p.ctypes.data_as(C.c_void_p),
                                         nn_c.ctypes.data_as(C.c_void_p), d2_c.ctypes.data_as(C.c_void_p)))
        return nn_p, d2_p, nn_c, d2_c

    # ---- headless renderer (include/fluidengine_ext.h; HIP engine only, no fallback)
    def render_setup(self, camera, lights):
        """fe_render_setup: a FeRenderCamera and a FeRenderLights (renderers/hip_renderer.py builds them); allocates or re-sizes the image buffers"""
        self._need_ext('render calls')
        self._ck(self.lib.fe_render_setup(self.h, C.byref(camera), C.sizeof(FeRenderCamera), C.byref(lights), C.sizeof(FeRenderLights)))
        self._render_res = (int(camera.width), int(camera.height))

    def render_set_colors(self, rgba, radius):
        """fe_render_set_colors: uint8 [N, 4] by particle id and the particles' world radius"""
        self._need_ext('render calls')
        c = np.ascontiguousarray(rgba, np.uint8)
        assert c.shape == (self.N, 4), c.shape
        self._ck(self.lib.fe_render_set_colors(self.h, c.ctypes.data_as(C.c_void_p), C.c_double(float(radius))))

    def render_set_points(self, set_id, xyz, rgba=(255, 255, 255, 255), radius=0.0):
        """fe_render_set_points: a static point set [n, 3] drawn with one colour and radius (ids N + set * FE_RENDER_MAX_POINTS + i); None removes it"""
        self._need_ext('render calls')
        if xyz is None:
            self._ck(self.lib.fe_render_set_points(self.h, int(set_id), None, 0, None, C.c_double(0.0)))
            return
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        c = np.ascontiguousarray(rgba, np.uint8).reshape(4)
        self._ck(self.lib.fe_render_set_points(self.h, int(set_id), p.ctypes.data_as(C.c_void_p), int(len(p)), c.ctypes.data_as(C.c_void_p), C.c_double(float(radius))))

    def render_frame(self, f):
        """fe_render_frame: enqueue the picture of frame f (does not wait)"""
        self._need_ext('render calls')
        self._ck(self.lib.fe_render_frame(self.h, int(f)))

    def render_set_volume(self, slot, source=FE_RENDER_VOL_NONE, index=0, rgba=(255, 255, 255, 255), voxels=None, T_mesh_to_voxels=None):
        """fe_render_set_volume: slot `slot` draws engine static `index` (FE_RENDER_VOL_STATIC), the posed mesh of effector `index` (_EFFECTOR) or
        the renderer's own copy of voxels [res]^3 with T_mesh_to_voxels (_OWN), in one colour (id N + sets + slot); FE_RENDER_VOL_NONE clears it"""
        self._need_ext('render calls')
        d, pv, keep = None, None, None
        if voxels is not None:
            keep, pv = self._r(voxels)
            if keep.ndim != 3 or not keep.shape[0] == keep.shape[1] == keep.shape[2]:
                raise FeEngineError('render_set_volume: voxels must be a cube')
            d = self.elib.FeSdfDesc()
            d.struct_size = C.sizeof(self.elib.FeSdfDesc)
            d.res = int(keep.shape[0])
            d.T_mesh_to_voxels[:] = [float(t) for t in np.asarray(T_mesh_to_voxels, np.float64).reshape(16)]
        c = np.ascontiguousarray(np.asarray(rgba, np.uint8).reshape(4))
        self._ck(self.lib.fe_render_set_volume(self.h, int(slot), int(source), int(index), None if d is None else C.byref(d), pv, c.ctypes.data_as(C.c_void_p)))

    def render_set_scene(self, scene):
        """fe_render_set_scene: a FeRenderScene, or None for no scene"""
        self._need_ext('render calls')
        self._ck(self.lib.fe_render_set_scene(self.h, None if scene is None else C.byref(scene), C.sizeof(FeRenderScene)))

    def render_scene_frame(self, f, s=0):
        """fe_render_scene_frame: enqueue the picture of frame f with the volumes and smoke frame s in it (does not wait)"""
        self._need_ext('render calls')
        self._ck(self.lib.fe_render_scene_frame(self.h, int(f), int(s)))

    def render_get(self, rgba=True, depth=False, ids=False):
        """fe_render_get: the last picture to the host -- (rgba uint8 [H, W, 4], depth float32 [H, W], id int32 [H, W]), None where not asked for"""
        self._need_ext('render calls')
        if getattr(self, '_render_res', None) is None:
            raise FeEngineError('render_get: no renderer: render_setup first')
        W, H = self._render_res
        a = np.zeros((H, W, 4), np.uint8) if rgba else None
        d = np.zeros((H, W), np.float32) if depth else None
        i = np.zeros((H, W), np.int32) if ids else None
        self._ck(self.lib.fe_render_get(self.h, *[None if t is None else t.ctypes.data_as(C.c_void_p) for t in (a, d, i)]))
        return a, d, i

    def render_get_dev(self, rgba=None, depth=None, ids=None):
        """fe_render_get_dev: the same into torch tensors on the engine's GPU (uint8 [H, W, 4], float32 [H, W], int32 [H, W]; None = skip).
        Enqueued on the engine's stream; sync() before torch reads them."""
        self._need_ext('render calls')
        import torch
        if getattr(self, '_render_res', None) is None:
            raise FeEngineError('render_get_dev: no renderer: render_setup first')
        W, H = self._render_res
        for name, t, shape, dt in (('rgba', rgba, (H, W, 4), torch.uint8), ('depth', depth, (H, W), torch.float32), ('ids', ids, (H, W), torch.int32)):
            if t is None:
                continue
            if not (t.is_cuda and t.device.index == self.device and tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous()):
                raise FeEngineError(f'render_get_dev: {name} must be a contiguous {dt} tensor of shape {shape} on cuda:{self.device}, '
                                    f'got {t.dtype} {tuple(t.shape)} on {t.device}')
        self._torch_fence(rgba, depth, ids)
        self._ck(self.lib.fe_render_get_dev(self.h, self._tptr(rgba), self._tptr(depth), self._tptr(ids)))

    # ---- liquids as a smoothed, translucent surface in that picture (include/fluidengine_ext.h: fe_surface_*)
    def surface_set(self, sel, params=None):
        """fe_surface_set: sel uint8 / bool [N] by particle id (non-zero: drawn as liquid) and a FeSurfaceParams; None or all zero switches it off"""
        self._need_ext('surface calls')
        if sel is None:
            self._ck(self.lib.fe_surface_set(self.h, None, None, 0))
            return
        s = np.ascontiguousarray(np.asarray(sel) != 0, np.uint8).reshape(-1)
        assert s.shape == (self.N,), s.shape
        self._ck(self.lib.fe_surface_set(self.h, s.ctypes.data_as(C.c_void_p), None if params is None else C.byref(params), C.sizeof(FeSurfaceParams)))

    def surface_frame(self, f, s=0):
        """fe_surface_frame: enqueue the picture render_scene_frame(f, s) would give, with the liquid surface (does not wait)"""
        self._need_ext('surface calls')
        self._ck(self.lib.fe_surface_frame(self.h, int(f), int(s)))

    def surface_get(self, z_raw=True, z_smooth=True, thickness=True):
        """fe_surface_get: the liquid layer of the last surface_frame -- (z_raw float32 [H, W], z_smooth float32 [H, W], thickness float64
        [H, W]), None where not asked for; +inf depth where there is no liquid"""
        self._need_ext('surface calls')
        if getattr(self, '_render_res', None) is None:
            raise FeEngineError('surface_get: no renderer: render_setup first')
        W, H = self._render_res
        a = np.zeros((H, W), np.float32) if z_raw else None
        b = np.zeros((H, W), np.float32) if z_smooth else None
        t = np.zeros((H, W), np.float64) if thickness else None
        self._ck(self.lib.fe_surface_get(self.h, *[None if v is None else v.ctypes.data_as(C.c_void_p) for v in (a, b, t)]))
        return a, b, t

    def surface_get_dev(self, z_raw=None, z_smooth=None, thickness=None):
        """fe_surface_get_dev: the same into torch tensors on the engine's GPU (float32, float32, float64, [H, W] each; None = skip).
        Enqueued on the engine's stream; sync() before torch reads them."""
        self._need_ext('surface calls')
        import torch
        if getattr(self, '_render_res', None) is None:
            raise FeEngineError('surface_get_dev: no renderer: render_setup first')
        W, H = self._render_res
        for name, t, dt in (('z_raw', z_raw, torch.float32), ('z_smooth', z_smooth, torch.float32), ('thickness', thickness, torch.float64)):
            if t is None:
                continue
            if not (t.is_cuda and t.device.index == self.device and tuple(t.shape) == (H, W) and t.dtype == dt and t.is_contiguous()):
                raise FeEngineError(f'surface_get_dev: {name} must be a contiguous {dt} tensor of shape {(H, W)} on cuda:{self.device}, '
                                    f'got {t.dtype} {tuple(t.shape)} on {t.device}')
        self._torch_fence(z_raw, z_smooth, thickness)
        self._ck(self.lib.fe_surface_get_dev(self.h, self._tptr(z_raw), self._tptr(z_smooth), self._tptr(thickness)))

    # ---- effectors
    def add_effector(self, *, type, action_dim, action_scale_v, action_scale_p, boundary, flux=0,
                     radius=0.0, inject_v=(0, 0, 0), inject_p=(0, 0, 0), locally_random=False,
                     randomize_inject_v=False, random_vector=None):
        d = self.elib.FeEffectorDesc()
        d.struct_size = C.sizeof(self.elib.FeEffectorDesc)
        d.type = int(type)
        d.action_dim = int(action_dim)
        sv = list(action_scale_v) + [1.0] * 8
        sp = list(action_scale_p) + [1.0] * 8
        d.action_scale_v[:] = [float(t) for t in sv[:8]]
        d.action_scale_p[:] = [float(t) for t in sp[:8]]
        d.boundary = boundary
        d.flux = int(flux)
        d.radius = float(radius)
        d.inject_v[:] = [float(t) for t in inject_v]
        d.inject_p[:] = [float(t) for t in inject_p]
        d.locally_random = int(bool(locally_random))
        d.randomize_inject_v = int(bool(randomize_inject_v))
        keep, prv = None, None
        if random_vector is not None:
            keep, prv = self._r(random_vector)
            assert keep.ndim == 3 and keep.shape[1] == flux and keep.shape[2] == 3
            d.random_length = keep.shape[0]
        e = self.lib.fe_add_effector(self.h, C.byref(d), prv)
        if e < 0:
            raise FeEngineError(self.lib.fe_last_error(self.h).decode())
        self._eff_action_dim[int(e)] = int(action_dim)
        return e

    def add_static(self, voxels, T_mesh_to_voxels, friction=0.0, softness=0.0):
        """statics.add_static (statics.py:14): one SDF collider for grid_op; returns its index."""
        keep, pv = self._r(voxels)
        assert keep.ndim == 3 and keep.shape[0] == keep.shape[1] == keep.shape[2]
        d = self.elib.FeSdfDesc()
        d.struct_size = C.sizeof(self.elib.FeSdfDesc)
        d.res = int(keep.shape[0])
        d.T_mesh_to_voxels[:] = [float(t) for t in np.asarray(T_mesh_to_voxels, np.float64).reshape(16)]
        d.friction = float(friction)
        d.softness = float(softness)
        i = self.lib.fe_add_static(self.h, C.byref(d), pv)
        if i < 0:
            raise FeEngineError(self.lib.fe_last_error(self.h).decode())
        return i

    # ---- AirCon strength / radius
    def eff_get_sr(self, e, f):
        s_, r_ = self.elib.real(), self.elib.real()
        self._ck(self.lib.fe_eff_get_sr(self.h, int(e), int(f), C.byref(s_), C.byref(r_)))
        return float(s_.value), float(r_.value)

    def eff_set_sr(self, e, f, s, r):
        self._ck(self.lib.fe_eff_set_sr(self.h, int(e), int(f), self.elib.real(float(s)), self.elib.real(float(r))))

    # ---- smoke field (smoke_field.py)
    def smoke_create(self, res=128, dt=0.03, solver_iters=500, q_dim=3, decay=0.99, max_steps_local=None, high_T=1.0, low_T=0.0,
                     lower_y=60, higher_y=68):
        c = self.elib.FeSmokeConfig()
        c.struct_size = C.sizeof(self.elib.FeSmokeConfig)
        c.res, c.solver_iters, c.q_dim, c.max_steps_local = int(res), int(solver_iters), int(q_dim), int(max_steps_local)
        c.dt, c.decay, c.high_T, c.low_T = float(dt), float(decay), float(high_T), float(low_T)
        c.lower_y, c.higher_y = int(lower_y), int(higher_y)
        self._ck(self.lib.fe_smoke_create(self.h, C.byref(c)))
        self.smoke_res, self.smoke_q_dim = int(res), int(q_dim)
        self._smoke_list_n = {}                              # (fe_smoke_create drops every cell list)

    def smoke_step(self, s, f):
        self._ck(self.lib.fe_smoke_step(self.h, int(s), int(f)))

    def smoke_step_grad(self, s, f):
        self._ck(self.lib.fe_smoke_step_grad(self.h, int(s), int(f)))

    def smoke_get_frame(self, s, fields=('v', 'q')):
        n, qd = self.smoke_res, self.smoke_q_dim
        shapes = dict(v=(n, n, n, 3), v_tmp=(n, n, n, 3), div=(n, n, n), p=(n, n, n), q=(n, n, n, qd))
        out = {k: np.zeros(shapes[k], self.dtype) for k in fields}
        ptr = [out[k].ctypes.data_as(C.c_void_p) if k in out else None for k in ('v', 'v_tmp', 'div', 'p', 'q')]
        self._ck(self.lib.fe_smoke_get_frame(self.h, int(s), *ptr))
        return out

    def smoke_set_frame(self, s, **arrays):
        keep = {k: np.ascontiguousarray(a, self.dtype) for k, a in arrays.items() if a is not None}
        ptr = [keep[k].ctypes.data_as(C.c_void_p) if k in keep else None for k in ('v', 'v_tmp', 'div', 'p', 'q')]
        self._ck(self.lib.fe_smoke_set_frame(self.h, int(s), *ptr))

    def smoke_get_grad(self, s):
        n, qd = self.smoke_res, self.smoke_q_dim
        gv, gq = np.zeros((n, n, n, 3), self.dtype), np.zeros((n, n, n, qd), self.dtype)
        self._ck(self.lib.fe_smoke_get_grad(self.h, int(s), gv.ctypes.data_as(C.c_void_p), gq.ctypes.data_as(C.c_void_p)))
        return gv, gq

    def smoke_add_grad(self, s, gv=None, gq=None):
        kv = None if gv is None else np.ascontiguousarray(gv, self.dtype)
        kq = None if gq is None else np.ascontiguousarray(gq, self.dtype)
        self._ck(self.lib.fe_smoke_add_grad(self.h, int(s), None if kv is None else kv.ctypes.data_as(C.c_void_p),
                                            None if kq is None else kq.ctypes.data_as(C.c_void_p)))

    def smoke_copy_frame(self, src, dst):
        self._ck(self.lib.fe_smoke_copy_frame(self.h, int(src), int(dst)))

    def smoke_copy_grad(self, src, dst):
        self._ck(self.lib.fe_smoke_copy_grad(self.h, int(src), int(dst)))

    def smoke_reset_grad(self):
        self._ck(self.lib.fe_smoke_reset_grad(self.h))

    def smoke_reset_grad_till_frame(self, s):
        self._ck(self.lib.fe_smoke_reset_grad_till_frame(self.h, int(s)))

    # ---- smoke-field reads that stay on the GPU (include/fluidengine_ext.h; HIP engine only, no fallback)
    def smoke_cells_set(self, list_id, cells):
        """fe_smoke_cells_set: list `list_id` = cells [n,3] of (i, j, k) (duplicates allowed; None or empty removes the list)"""
        self._need_ext('smoke-field reads')
        cells = None if cells is None else np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
        n = 0 if cells is None else int(cells.shape[0])
        self._ck(self.lib.fe_smoke_cells_set(self.h, int(list_id), cells.ctypes.data_as(C.c_void_p) if n else None, n))
        self._smoke_list_n[int(list_id)] = n

    def _smoke_n(self, list_id):
        return self._smoke_list_n.get(int(list_id), 0)

    def smoke_cells_get(self, list_id, s):
        """{'v' [n,3], 'q' [n,q_dim]}: the listed cells' rows of smoke frame s -- n rows are copied to the host, not the fields"""
        self._need_ext('smoke-field reads')
        n = self._smoke_n(list_id)
        out = {'v': np.zeros((n, 3), self.dtype), 'q': np.zeros((n, getattr(self, 'smoke_q_dim', 1)), self.dtype)}
        self._ck(self.lib.fe_smoke_cells_get(self.h, int(list_id), int(s), out['v'].ctypes.data_as(C.c_void_p), out['q'].ctypes.data_as(C.c_void_p)))
        return out

    def smoke_cells_get_dev(self, list_id, s, v=None, q=None):
        """the same into float32 torch tensors on the engine's GPU (v [n,3], q [n,q_dim]; None = skip); enqueued, does not wait"""
        self._need_ext('smoke-field reads')
        import torch
        n = self._smoke_n(list_id)
        for name, t, shape in (('v', v, (n, 3)), ('q', q, (n, getattr(self, 'smoke_q_dim', 1)))):
            if t is None:
                continue
            if not (t.is_cuda and t.device.index == self.device and tuple(t.shape) == shape and t.dtype == torch.float32 and t.is_contiguous()):
                raise FeEngineError(f'smoke_cells_get_dev: {name} must be a contiguous float32 tensor of shape {shape} on cuda:{self.device}, '
                                    f'got {t.dtype} {tuple(t.shape)} on {t.device}')
        self._torch_fence(v, q)
        self._ck(self.lib.fe_smoke_cells_get_dev(self.h, int(list_id), int(s), self._tptr(v), self._tptr(q)))

    def smoke_cells_add_grad(self, list_id, s, gv=None, gq=None):
        """fe_smoke_cells_add_grad: row i of gv [n,3] / gq [n,q_dim] is added to the v / q adjoint of cell i of list `list_id` in smoke frame
        s (None = skip); rows of a cell listed several times are summed in list order in fp32 first.  numpy arrays go through the host entry
        (staged, waits); contiguous float32 torch tensors on the engine's GPU through the _dev entry (enqueued, does not wait: the
        tensors are kept alive here until the next call, and the caller leaves them unchanged until an engine call that waits)."""
        self._need_ext('smoke-field reads')
        n, qd = self._smoke_n(list_id), getattr(self, 'smoke_q_dim', 1)
        dev = [t is not None and hasattr(t, 'data_ptr') and not isinstance(t, np.ndarray) for t in (gv, gq)]
        if not any(dev):
            kv, pv = self._r(gv, (n, 3)); kq, pq = self._r(gq, (n, qd))
            self._ck(self.lib.fe_smoke_cells_add_grad(self.h, int(list_id), int(s), pv, pq))
            return
        import torch
        for name, t, shape in (('gv', gv, (n, 3)), ('gq', gq, (n, qd))):
            if t is None:
                continue
            if not (hasattr(t, 'is_cuda') and t.is_cuda and t.device.index == self.device and tuple(t.shape) == shape and t.dtype == torch.float32
                    and t.is_contiguous()):
                raise FeEngineError(f'smoke_cells_add_grad: {name} must be a contiguous float32 tensor of shape {shape} on cuda:{self.device} '
                                    f'(or both numpy arrays), got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))} on {getattr(t, "device", "the host")}')
        self._torch_fence(gv, gq)
        self._smoke_scatter_keep = (gv, gq)
        self._ck(self.lib.fe_smoke_cells_add_grad_dev(self.h, int(list_id), int(s), self._tptr(gv), self._tptr(gq)))

    # ---- Circulation's observation vector and its cotangent, one device call each (fe_smoke_obs_*)
    FE_SMOKE_OBS_STATE = 9

    def smoke_obs_size(self, list_id):
        """the length of the vector of fe_smoke_obs_*: 9 + n (3 + q_dim)"""
        return self.FE_SMOKE_OBS_STATE + self._smoke_n(list_id) * (3 + getattr(self, 'smoke_q_dim', 1))

    def smoke_obs_get(self, list_id, s, eff, f, out=None):
        """fe_smoke_obs_get: [pos 3, quat 4, s, r] of AirCon `eff` at local frame f, then the v rows and the q rows of list `list_id` in smoke
        frame s, as one vector from one launch.  out=None: a numpy array (the host entry; waits).  out a contiguous float32 torch tensor
        [smoke_obs_size] on the engine's GPU: the _dev entry (enqueued, does not wait); returns out."""
        self._need_ext('smoke-field reads')
        n = self.smoke_obs_size(list_id)
        if out is None:
            out = np.zeros((n,), self.dtype)
            self._ck(self.lib.fe_smoke_obs_get(self.h, int(list_id), int(s), int(eff), int(f), out.ctypes.data_as(C.c_void_p), n))
            return out
        self._dev_tensor('smoke_obs_get', 'out', out, (n,))
        self._torch_fence(out)
        self._ck(self.lib.fe_smoke_obs_get_dev(self.h, int(list_id), int(s), int(eff), int(f), self._tptr(out), n))
        return out

    def smoke_obs_add_grad(self, list_id, s, eff, f, g):
        """fe_smoke_obs_add_grad: the adjoint of smoke_obs_get in one launch.  g [smoke_obs_size]: its v / q rows go to the smoke adjoint of
        frame s at the listed cells (as smoke_cells_add_grad), g[:7] to the pose adjoint and g[7], g[8] to the s / r adjoint of AirCon `eff`
        at local frame f.  A numpy array goes through the host entry (staged, waits); a contiguous float32 torch tensor on the engine's GPU
        through the _dev entry (enqueued, does not wait: it is kept alive here until the next call, and the caller leaves it unchanged
        until an engine call that waits)."""
        self._need_ext('smoke-field reads')
        n = self.smoke_obs_size(list_id)
        if g is None:
            raise FeEngineError('smoke_obs_add_grad: g is None')
        if hasattr(g, 'data_ptr') and not isinstance(g, np.ndarray):
            self._dev_tensor('smoke_obs_add_grad', 'g', g, (n,))
            self._torch_fence(g)
            self._smoke_obs_keep = g
            self._ck(self.lib.fe_smoke_obs_add_grad_dev(self.h, int(list_id), int(s), int(eff), int(f), self._tptr(g), n))
            return
        k, p = self._r(g, (n,))
        self._ck(self.lib.fe_smoke_obs_add_grad(self.h, int(list_id), int(s), int(eff), int(f), p, n))

    def eff_add_sr_grad(self, e, f, gs, gr):
        """fe_eff_add_sr_grad: gsa[f] += gs, gra[f] += gr of AirCon e (the adjoints of its strength and radius)"""
        self._need_ext(self._POLICY_IO)
        self._ck(self.lib.fe_eff_add_sr_grad(self.h, int(e), int(f), self.elib.real(float(gs)), self.elib.real(float(gr))))

    def eff_get_sr_grad(self, e, f):
        """fe_eff_get_sr_grad: (gsa[f], gra[f]) of AirCon e"""
        self._need_ext(self._POLICY_IO)
        gs, gr = self.elib.real(), self.elib.real()
        self._ck(self.lib.fe_eff_get_sr_grad(self.h, int(e), int(f), C.byref(gs), C.byref(gr)))
        return float(gs.value), float(gr.value)

    def smoke_loss_alloc(self, max_loss_steps):
        """fe_smoke_loss_alloc: step_loss[max_loss_steps], fp64 on the device, zeroed"""
        self._need_ext('smoke-field reads')
        self._ck(self.lib.fe_smoke_loss_alloc(self.h, int(max_loss_steps)))

    def smoke_loss_set(self, list_id, target, weight=None, comp=0, kind=FE_SMOKE_L1):
        """fe_smoke_loss_set: the detectors are the cells of list `list_id` (no duplicates); target [n], weight [n] or None (= 1), fp64"""
        self._need_ext('smoke-field reads')
        n = self._smoke_n(list_id)
        t = np.ascontiguousarray(target, np.float64).reshape(-1)
        w = None if weight is None else np.asarray(weight, np.float64).reshape(-1)
        if w is not None and w.size == 1:
            w = np.full((max(n, 1),), w[0])                      # (a scalar: every detector)
        if w is not None and n and w.size != n:
            raise FeEngineError(f'smoke_loss_set: {w.size} weights for a list of {n} cells')
        w = None if w is None else np.ascontiguousarray(w)
        if n and t.size != n:
            raise FeEngineError(f'smoke_loss_set: {t.size} targets for a list of {n} cells')
        self._ck(self.lib.fe_smoke_loss_set(self.h, int(list_id), int(comp), int(kind), t.ctypes.data_as(C.c_void_p),
                                            None if w is None else w.ctypes.data_as(C.c_void_p)))

    def smoke_loss_clear(self):
        self._need_ext('smoke-field reads')
        self._ck(self.lib.fe_smoke_loss_clear(self.h))

    def smoke_loss_step(self, s_loss, s):
        """fe_smoke_loss_step: step_loss[s_loss] += the detector loss of smoke frame s (enqueued; does not wait)"""
        self._need_ext('smoke-field reads')
        self._ck(self.lib.fe_smoke_loss_step(self.h, int(s_loss), int(s)))

    def smoke_loss_step_grad(self, s_loss, s, scale=1.0):
        """fe_smoke_loss_step_grad: q.grad[s] += (float)(scale * d value / d q) at the detectors (enqueued; does not wait)"""
        self._need_ext('smoke-field reads')
        self._ck(self.lib.fe_smoke_loss_step_grad(self.h, int(s_loss), int(s), C.c_double(float(scale))))

    def smoke_loss_get(self, n, s0=0):
        """step_loss[s0:s0+n] as a fp64 array.  Waits for the engine's stream."""
        self._need_ext('smoke-field reads')
        sl = np.zeros((n,), np.float64)
        self._ck(self.lib.fe_smoke_loss_get(self.h, int(s0), int(n), sl.ctypes.data_as(C.c_void_p)))
        return sl

    def smoke_summary(self, s):
        """fe_smoke_summary: a dict of the fields of FeSmokeSummary (q_sum, q_min, q_max as fp64 arrays of 3)"""
        self._need_ext('smoke-field reads')
        rec = FeSmokeSummary()
        self._ck(self.lib.fe_smoke_summary(self.h, int(s), C.byref(rec), C.sizeof(FeSmokeSummary)))
        return {k: (np.array(getattr(rec, k), np.float64) if k in ('q_sum', 'q_min', 'q_max') else getattr(rec, k)) for k, _ in FeSmokeSummary._fields_}

    def eff_set_mesh(self, e, voxels, T_mesh_to_voxels, friction=0.0, softness=0.0):
        """Rigid.setup_mesh (rigid.py:19-24): effector e becomes a moving SDF collider."""
        keep, pv = self._r(voxels)
        assert keep.ndim == 3 and keep.shape[0] == keep.shape[1] == keep.shape[2]
        d = self.elib.FeSdfDesc()
        d.struct_size = C.sizeof(self.elib.FeSdfDesc)
        d.res = int(keep.shape[0])
        d.T_mesh_to_voxels[:] = [float(t) for t in np.asarray(T_mesh_to_voxels, np.float64).reshape(16)]
        d.friction = float(friction)
        d.softness = float(softness)
        self._ck(self.lib.fe_eff_set_mesh(self.h, int(e), C.byref(d), pv))

    def eff_set_act_range(self, e, act_range):
        k, p = self._i(act_range)
        self._ck(self.lib.fe_eff_set_act_range(self.h, int(e), p, int(k.shape[0])))

    def eff_get_state(self, e, f):
        s = np.zeros((8,), self.dtype)
        self._ck(self.lib.fe_eff_get_state(self.h, int(e), int(f), s.ctypes.data_as(C.c_void_p)))
        return s

    def eff_set_state(self, e, f, state8):
        k, p = self._r(state8, (8,))
        self._ck(self.lib.fe_eff_set_state(self.h, int(e), int(f), p))

    def eff_get_vw(self, e, f):
        v = np.zeros((3,), self.dtype); w = np.zeros((3,), self.dtype)
        self._ck(self.lib.fe_eff_get_vw(self.h, int(e), int(f), v.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)))
        return v, w

    def eff_set_vw(self, e, f, v, w):
        k0, pv = self._r(v, (3,)); k1, pw = self._r(w, (3,))
        self._ck(self.lib.fe_eff_set_vw(self.h, int(e), int(f), pv, pw))

    def eff_set_action(self, e, s, s_global, n_substeps, action):
        k, p = self._r(action)
        self._ck(self.lib.fe_eff_set_action(self.h, int(e), int(s), int(s_global), int(n_substeps), p))

    def eff_set_action_grad(self, e, s, s_global, n_substeps):
        self._ck(self.lib.fe_eff_set_action_grad(self.h, int(e), int(s), int(s_global), int(n_substeps)))

    def eff_apply_action_p(self, e, action_p):
        k, p = self._r(action_p)
        self._ck(self.lib.fe_eff_apply_action_p(self.h, int(e), p))

    def eff_apply_action_p_grad(self, e):
        self._ck(self.lib.fe_eff_apply_action_p_grad(self.h, int(e)))

    def eff_get_action_grad(self, e, s, n, action_dim):
        g = np.zeros((n + 1, action_dim), self.dtype)
        self._ck(self.lib.fe_eff_get_action_grad(self.h, int(e), int(s), int(n), g.ctypes.data_as(C.c_void_p)))
        return g

    def agent_copy_frame(self, src, dst):
        self._ck(self.lib.fe_agent_copy_frame(self.h, int(src), int(dst)))

    def agent_copy_grad(self, src, dst):
        self._ck(self.lib.fe_agent_copy_grad(self.h, int(src), int(dst)))

    def agent_reset_grad_till_frame(self, f):
        self._ck(self.lib.fe_agent_reset_grad_till_frame(self.h, int(f)))

    def agent_set_collector(self, boundary=None, mat=-1):
        """collector_act_kernel (agent_pouring.py:30-41 every material, agent_jetbot.py:33-43 one material)."""
        self._ck(self.lib.fe_agent_set_collector(self.h, C.byref(boundary) if boundary is not None else None, int(mat)))

    # ---- loss
    def loss_alloc(self, max_loss_steps):
        self._ck(self.lib.fe_loss_alloc(self.h, int(max_loss_steps)))

    def loss_set_target(self, s, x):
        k, p = self._r(x, (self.N, 3))
        self._ck(self.lib.fe_loss_set_target(self.h, int(s), p))

    def loss_clear(self):
        self._ck(self.lib.fe_loss_clear(self.h))

    def loss_step(self, s, f, matching_mat, weight):
        self._ck(self.lib.fe_loss_step(self.h, int(s), int(f), int(matching_mat), self.elib.real(weight)))

    def loss_step_grad(self, s, f, matching_mat, weight, step_loss_grad):
        self._ck(self.lib.fe_loss_step_grad(self.h, int(s), int(f), int(matching_mat), self.elib.real(weight),
                                            self.elib.real(step_loss_grad)))

    def loss_get(self, n):
        a = np.zeros((n,), self.dtype)
        self._ck(self.lib.fe_loss_get(self.h, a.ctypes.data_as(C.c_void_p), int(n)))
        return a

    # ---- measurement
    def get_stats(self, f):
        st = FeStats()
        self._ck(self.lib.fe_get_stats(self.h, int(f), C.byref(st)))
        return {k: getattr(st, k) for k, _ in FeStats._fields_}

    def get_work_stats(self, f, launches=False):
        """The work list of frame f's particle order.  launches=True adds `grid_launch` / `grid_grad_launch`, the records of the frame's last separate grid-kernel
        launches: unlike the rest they are no property of the order -- what a forward launch was sized from depends on whether the sort's length had reached the
        host when it was enqueued -- so two runs of the same scene agree on everything but them."""
        out = (C.c_longlong * 30)()
        out[24] = out[27] = -1                               # (a library that writes a shorter list: no grid-launch record)
        if hasattr(self.lib, 'fe_get_work_stats_n'):         # (the counted form: an A/B library of an earlier round writes its own, shorter list)
            self._ck(self.lib.fe_get_work_stats_n(self.h, int(f), out, 30))
        else:
            self._ck(self.lib.fe_get_work_stats(self.h, int(f), out))
        keys = ('n_items', 'tail_start', 'n_active_blocks', 'n_multi_item_workgroups', 'n_single_item_blocks')
        d = {k: int(out[i]) for i, k in enumerate(keys)}
        d['items_by_size'] = {k: int(out[5 + i]) for i, k in enumerate(('1', '2-4', '5-8', '9-16', '17-32', '33-64', '65-128'))}
        d['n_occupied_blocks'] = int(out[12])
        d['n_loose_particles'] = int(out[13])            # particles of blocks without a work item (engine option loose_max)
        d['n_quad_items'] = int(out[14])                 # single-item blocks of <= quad_max particles: four to a workgroup, one wave each ...
        d['n_quad_units'] = int(out[15])                 # ... when the order's unit list holds quad units at all (engine option quad_min_units): how many
        d['n_scatter_units'], d['n_gather_units'] = int(out[16]), int(out[17])     # work units of the two unit lists: the workgroups of a scatter / gather launch that have something to do
        d['packed'] = bool(out[18])                      # the scatter list has no idle halves (engine options pack_units, quad_fit)
        d['n_leftover_items'] = int(out[19]) + int(out[20])
        d['n_split9_waves'], d['n_split3_waves'] = int(out[21]), int(out[22])      # waves of <= 7 / 8..21 particles: nine / three lanes per particle (engine option lane_split)
        # the separate grid kernels' launches of frame f (fe_grid_launch.h): workgroups, the active-list length they were sized from (-1: fixed geometry) and
        # where it came from ('none', 'lagged': the newest sort that had reported, 'exact': the frame's own order, 'forced': option grid_hint)
        if launches:
            kinds = ('none', 'lagged', 'exact', 'forced')
            d['grid_launch'] = {'wgs': int(out[23]), 'hint': int(out[24]), 'kind': kinds[int(out[25]) & 3]}
            d['grid_grad_launch'] = {'wgs': int(out[26]), 'hint': int(out[27]), 'kind': kinds[int(out[28]) & 3]}
        return d

    def timer_start(self):
        self._ck(self.lib.fe_timer_start(self.h))

    def timer_stop_ms(self):
        ms = self.lib.fe_timer_stop_ms(self.h)
        if ms < 0:
            raise FeEngineError(self.lib.fe_last_error(self.h).decode())
        return ms

    def profile_enable(self, on):
        self._ck(self.lib.fe_profile_enable(self.h, int(bool(on))))

    def profile_read(self, cap=32):
        buf = C.create_string_buffer(4096)
        ms = (C.c_double * cap)()
        cnt = (C.c_longlong * cap)()
        n = self.lib.fe_profile_read(self.h, buf, 4096, ms, cnt, cap)
        names = buf.value.decode().split('\n') if n > 0 else []
        return {names[i]: (ms[i], cnt[i]) for i in range(min(n, len(names)))}
