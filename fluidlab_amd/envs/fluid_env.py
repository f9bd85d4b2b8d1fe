"""FluidEnv -- the task-environment base class (fluidlab/envs/fluid_env.py) without the gym dependency
(gym is not in this image): reset/step/seed and Box-like spaces are provided here."""
import numpy as np

import fluidlab_amd.utils.misc as misc_utils
from fluidlab_amd.configs.macros import DTYPE_NP, WATER
from fluidlab_amd.fluidengine.taichi_env import TaichiEnv


class Box:
    def __init__(self, low, high, shape, dtype=DTYPE_NP):
        self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype

    def sample(self):
        return np.random.uniform(self.low, self.high, self.shape).astype(self.dtype)


class FluidEnv:
    # (class-level defaults: task envs have constructors of their own)
    _device_obs = False                                          # enable_device_obs(): _get_obs gathers its particles on the GPU
    renderer_type = None                                         # 'HIP': build_env() calls setup_renderer()
    _diagnostics = False                                         # enable_diagnostics(): step() reports the new frame's summary in info
    _contact_info = False                                        # enable_contact_info(): step() reports the step's contact wrenches in info
    _field_obs = None                                            # enable_field_obs(): the fields _get_obs appends (dicts: spec, sel, channels)
    _field_obs_particles = True                                  # ... and whether the particle rows stay in the vector

    def __init__(self, version=0, loss=True, loss_type='diff', seed=None, renderer_type=None, **engine_kwargs):
        if seed is not None:
            self.seed(seed)
        self.horizon = 500
        self.horizon_action = 500
        self.target_file = None
        self._n_obs_ptcls_per_body = 200
        self.loss = loss
        self.loss_type = loss_type
        self.renderer_type = renderer_type
        self.action_range = np.array([-1.0, 1.0])
        self.taichi_env = TaichiEnv(**engine_kwargs)
        self.build_env()
        self.gym_misc()

    def seed(self, seed):
        misc_utils.set_random_seed(seed)

    #: the scene-description hooks a task env overrides, in the order the scene is assembled (fluid_env.py:35-49)
    SETUP_ORDER = ('setup_agent', 'setup_statics', 'setup_bodies', 'setup_smoke_field', 'setup_boundary')

    def build_env(self):
        for hook in self.SETUP_ORDER:
            getattr(self, hook)()
        if self.loss:
            self.setup_loss()
        self.taichi_env.build()
        if self.renderer_type is not None:                       # 'HIP': the headless particle renderer; anything else raises NotImplementedError there
            self.setup_renderer()
        self._init_state = self.taichi_env.get_state()           # reset() returns here
        print(f'===>  {type(self).__name__} built successfully.')

    def _nothing(self):
        """default of every optional hook"""

    setup_agent = setup_statics = setup_smoke_field = setup_boundary = setup_loss = _nothing

    def setup_renderer(self):
        """renderer_type='HIP': the renderer's own default camera and lights (a task env overrides this with its scene's)"""
        self.taichi_env.setup_renderer(type=self.renderer_type)

    def render(self, mode='human'):
        """mode='rgb_array': uint8 [H, W, 3] of the current frame (fluid_env.py:140-141); needs renderer_type='HIP'"""
        return self.taichi_env.render(mode)

    def setup_bodies(self):
        """the base class' demo scene: a water cube and a water ball"""
        self.taichi_env.add_body(type='cube', lower=(0.2, 0.2, 0.2), upper=(0.4, 0.4, 0.4), material=WATER)
        self.taichi_env.add_body(type='ball', center=(0.6, 0.3, 0.6), radius=0.1, material=WATER)

    def gym_misc(self):
        if self.loss_type == 'default':
            self.horizon = self.horizon_action
        obs = self.reset()
        self.observation_space = Box(DTYPE_NP(-np.inf), DTYPE_NP(np.inf), obs.shape)
        agent = self.taichi_env.agent
        self.action_space = Box(DTYPE_NP(self.action_range[0]), DTYPE_NP(self.action_range[1]), (agent.action_dim,)) if agent is not None else None

    def reset(self):
        self.taichi_env.set_state(**self._init_state)
        return self._get_obs()

    def _obs_ids(self):
        """per body the particle ids _get_obs keeps (particle_ids[::step_size]), and where each body's rows start in their concatenation"""
        bodies = self.taichi_env.particles['bodies']
        ids, start = [], [0]
        for body_id in range(bodies['n']):
            step_size = max(1, bodies['n_particles'][body_id] // self._n_obs_ptcls_per_body)
            ids.append(np.asarray(bodies['particle_ids'][body_id])[::step_size])
            start.append(start[-1] + len(ids[-1]))
        return ids, start

    def enable_device_obs(self):
        """From here on _get_obs() reads only the particles it keeps, gathered on the GPU (engine observation list), instead of downloading
        the whole frame.  The observation vector is the same.  HIP engine only."""
        if self.taichi_env.particles is None:
            return
        ids, self._obs_start = self._obs_ids()
        self.taichi_env.set_obs_particles(np.concatenate(ids) if ids else np.zeros((0,), np.int32))
        self._device_obs = True

    def enable_field_obs(self, fields, particles=True):
        """From here on _get_obs() appends Eulerian observations -- small grids of how much material is where and how it is moving -- after
        everything it builds today, so existing slices keep their place.  fields: a list of dict(lower, upper, n, mat=None, body=None,
        channels=4): n cells per axis (1 = projected along that axis) over the box [lower, upper], from the used particles of material
        `mat` and / or body `body` (None: all), with 1 channel (density) or 4 (density, momentum x y z; a particle's mass taken as 1).
        Each field is flattened [channels, n0, n1, n2].  particles=False leaves the particle rows out of the vector.  The values do not
        depend on the particles' order.  With enable_device_obs() on the HIP engine the fields are rasterised and differentiated in the
        engine (include/fluidengine_ext.h: fe_field_obs_*); otherwise from the downloaded frame by term_program.field_obs_of_points, with
        the same fixed point, on every engine.  None or an empty list turns the feature off."""
        from fluidlab_amd.fluidengine.losses.term_program import DensityField, Sel
        te = self.taichi_env
        if te.particles is None:
            raise RuntimeError('enable_field_obs: the scene has no particles')
        out = []
        for fd in (fields or []):
            fd = dict(fd)
            lower, upper = np.asarray(fd.pop('lower'), np.float64), np.asarray(fd.pop('upper'), np.float64)
            n = tuple(int(v) for v in fd.pop('n'))
            mat, body, channels = fd.pop('mat', None), fd.pop('body', None), int(fd.pop('channels', 4))
            assert not fd, f'enable_field_obs: unknown keys {sorted(fd)}'
            assert lower.shape == upper.shape == (3,) and len(n) == 3 and all(v >= 1 for v in n) and channels in (1, 4), (lower, upper, n, channels)
            cell = [float((upper[a] - lower[a]) / n[a]) if n[a] > 1 else (float(upper[a] - lower[a]) if upper[a] > lower[a] else 1.0) for a in range(3)]
            assert all(c > 0 for c in cell), f'enable_field_obs: upper must lie above lower on every unprojected axis, got {lower} {upper}'
            lo, hi = 0, te.n_particles
            if body is not None:                                 # a body's particles are one range of ids
                ids = np.asarray(te.particles['bodies']['particle_ids'][int(body)])
                lo, hi = int(ids.min()), int(ids.max()) + 1
                assert hi - lo == len(ids), f'enable_field_obs: the particle ids of body {body} are not one range'
            out.append(dict(spec=DensityField(tuple(float(v) for v in lower), tuple(cell), n), sel=Sel(lo, hi, -1 if mat is None else int(mat), True), channels=channels))
        te.set_field_obs([(d['spec'], d['sel'], d['channels']) for d in out])
        self._field_obs = out or None
        self._field_obs_particles = bool(particles) or not out

    def boundary_fields(self, n, channels=4):
        """what `run.py --closed_loop --field_obs N` observes: a top-down n x 1 x n field over the scene's boundary box (a cylinder's
        bounding box) for every liquid material of the scene, at most FE_FIELD_OBS_MAX of them"""
        from fluidlab_amd import _capi
        from fluidlab_amd.configs.macros import MAT_CLASS, MAT_LIQUID
        sim = self.taichi_env.simulator
        b = sim.engine.cfg.boundary
        lower, upper = [float(q) for q in b.lower], [float(q) for q in b.upper]
        if int(b.type) == _capi.FE_BOUNDARY_CYLINDER:
            (cx, cz), r = [float(q) for q in b.xz_center], float(b.xz_radius)
            lower[0], upper[0], lower[2], upper[2] = cx - r, cx + r, cz - r, cz + r
        mats = [m for m in sorted(set(int(q) for q in np.asarray(sim._mat_np))) if MAT_CLASS[m] == MAT_LIQUID]
        return [dict(lower=tuple(lower), upper=tuple(upper), n=(int(n), 1, int(n)), mat=m, channels=int(channels)) for m in mats[:_capi.FE_FIELD_OBS_MAX]]

    def _field_obs_on_device(self):
        return bool(self._device_obs) and self.taichi_env.simulator.engine.elib.has_ext

    def _field_obs_values(self, f=None):
        """the field blocks of the observation vector, flattened, in the engine's dtype"""
        if not self._field_obs:
            return []
        te = self.taichi_env
        dev = self._field_obs_on_device()
        return [np.asarray(te.field_obs(f, k, device=dev)).reshape(-1).astype(te.simulator.engine.dtype) for k in range(len(self._field_obs))]

    def enable_scene_render(self, **kwargs):
        """From here on render() / render_buffers() show what the fluid touches as well: the SDF colliders of the statics and the Rigid
        effectors, and the smoke field of a scene that has one (HIPRenderer.enable_scene takes the keywords).  Off by default; needs
        renderer_type='HIP'."""
        self.taichi_env.enable_scene_render(**kwargs)

    def enable_liquid_surface(self, **kwargs):
        """From here on render() / render_buffers() draw the liquid particles (material class MAT_LIQUID, the reference's GL renderer's rule) as
        one smoothed, translucent surface over the rest of the picture (HIPRenderer.enable_liquid_surface takes the keywords).  Off by default,
        so that existing pictures do not change; needs renderer_type='HIP'."""
        self.taichi_env.enable_liquid_surface(**kwargs)

    def enable_device_loss(self):
        """From here on the task loss of a HostLoss environment (GatheringEasy, GatheringO, Pouring, Transporting, Mixing) is evaluated and
        differentiated in the engine instead of through torch on downloaded positions.  The values agree to fp64 rounding.  HIP engine only.
        Circulation's CirculationLoss has a device road of its own (the detector sum over the smoke field) behind the same call."""
        self.taichi_env.enable_device_loss()

    def enable_diagnostics(self):
        """From here on step() fills info with courant, kinetic, n_used and n_nonfinite of the new frame (reduced on the GPU) and ends the
        episode when a used particle holds a non-finite value.  HIP engine only."""
        self._diagnostics = True

    def enable_contact_info(self):
        """From here on step() puts info['contact'] = TaichiEnv.contact_wrench(): per collider (the tool's effectors, then the statics) the
        force and torque the fluid put on it during the step, replayed on the GPU, with the share of substeps it covers.  The observation
        vector does not change.  Off by default.  HIP engine only."""
        self._contact_info = True

    def _get_obs(self):
        """fluid_env.py:102-129"""
        if self._device_obs:
            state = self.taichi_env.get_obs_RL()
            obs = []
            for b in range(len(self._obs_start) - 1 if self._field_obs_particles else 0):
                lo, hi = self._obs_start[b], self._obs_start[b + 1]
                obs += [state['x'][lo:hi].flatten(), state['v'][lo:hi].flatten(), state['used'][lo:hi].flatten()]
            if 'agent' in state:
                obs += state['agent']
            return np.concatenate(obs + self._field_obs_values())
        state = self.taichi_env.get_state_RL()
        obs = []
        if 'x' in state and self._field_obs_particles:
            bodies = self.taichi_env.particles['bodies']
            for body_id in range(bodies['n']):
                ids = bodies['particle_ids'][body_id]
                step_size = max(1, bodies['n_particles'][body_id] // self._n_obs_ptcls_per_body)
                obs += [state['x'][ids][::step_size].flatten(), state['v'][ids][::step_size].flatten(), state['used'][ids][::step_size].flatten()]
        if 'agent' in state:
            obs += state['agent']
        return np.concatenate(obs + self._field_obs_values())

    # ---- the observation vector's layout and its cotangent (closed-loop policies: optimizer/closed_loop.py)
    def obs_layout(self):
        """The slices of the vector _get_obs() builds, from the same _obs_ids() on both observation roads:
          'bodies'  per body {'x', 'v', 'used': slices, 'ids': the particle ids of its rows, 'rows': (lo, hi) in their concatenation};
          'agent'   per effector the slice of its pose (pos 3, quat 4);
          'extra'   per effector the slice of what its state holds beyond the pose (an Injector's act_id, an AirCon's s and r), or None;
          'fields'  with enable_field_obs() on: per field {'slice', 'shape': (channels, n0, n1, n2), 'channels'}, behind everything else
                    ('bodies' is empty with particles=False);
          'size'    the length of the vector."""
        te = self.taichi_env
        ids, start = self._obs_ids() if te.particles is not None and self._field_obs_particles else ([], [0])
        at, bodies = 0, []
        for b, pid in enumerate(ids):
            n = len(pid)
            bodies.append(dict(x=slice(at, at + 3 * n), v=slice(at + 3 * n, at + 6 * n), used=slice(at + 6 * n, at + 7 * n),
                               ids=np.asarray(pid, np.int32), rows=(start[b], start[b + 1])))
            at += 7 * n
        agent, extra = [], []
        for e in (te.agent.effectors if te.agent is not None else []):
            agent.append(slice(at, at + 7))
            extra.append(slice(at + 7, at + e.state_dim) if e.state_dim > 7 else None)
            at += e.state_dim
        if not self._field_obs:
            return dict(bodies=bodies, agent=agent, extra=extra, size=at)
        fields = []
        for d in self._field_obs:
            shape = (d['channels'],) + d['spec'].shape
            fields.append(dict(slice=slice(at, at + int(np.prod(shape))), shape=shape, channels=d['channels']))
            at += int(np.prod(shape))
        return dict(bodies=bodies, agent=agent, extra=extra, fields=fields, size=at)

    def _dense_obs_grad(self, g_obs, dtype=np.float32, layout=None):
        """the dense road's arrays: (gx, gv) [N, 3] in `dtype`, the x / v slices of g_obs added row by row, in list order, at their particles"""
        layout = self.obs_layout() if layout is None else layout
        N = self.taichi_env.n_particles
        gx, gv = np.zeros((N, 3), dtype), np.zeros((N, 3), dtype)
        g = np.asarray(g_obs).reshape(-1)
        for b in layout['bodies']:
            np.add.at(gx, b['ids'], g[b['x']].reshape(-1, 3).astype(dtype))
            np.add.at(gv, b['ids'], g[b['v']].reshape(-1, 3).astype(dtype))
        return gx, gv

    def obs_backward(self, g_obs, f=None):
        """Route the cotangent of an observation vector into the simulation: the x / v slices are added to the particle adjoint of local
        frame f (default: the current frame) at the observed particles, the `used` slices are dropped, the pose slices go to the
        effectors' state adjoints, the field slices (enable_field_obs) to the adjoint of their fields -- in the engine with
        enable_device_obs() on the HIP engine, otherwise through term_program.field_obs_grad_of_points and add_grad.  With enable_device_obs() on the HIP engine only the listed rows travel (a torch tensor on the engine's
        GPU does not leave it); otherwise dense [N, 3] arrays are built on the host and handed to add_grad, which every engine has.
        An engine without the extension has no entry for the pose adjoint: a non-zero pose cotangent raises there."""
        te = self.taichi_env
        sim = te.simulator
        f = sim.cur_substep_local if f is None else int(f)
        layout = self.obs_layout()
        on_gpu = hasattr(g_obs, 'data_ptr') and getattr(g_obs, 'is_cuda', False)
        g = g_obs.detach().reshape(-1) if hasattr(g_obs, 'detach') else np.asarray(g_obs).reshape(-1)
        assert g.shape[0] == layout['size'], f"obs_backward: the cotangent has {g.shape[0]} entries, the observation {layout['size']}"
        if layout['bodies']:
            if self._device_obs and sim.engine.elib.has_ext:
                if on_gpu:
                    import torch
                    gx = torch.cat([g[b['x']] for b in layout['bodies']]).reshape(-1, 3).to(torch.float32).contiguous()
                    gv = torch.cat([g[b['v']] for b in layout['bodies']]).reshape(-1, 3).to(torch.float32).contiguous()
                else:
                    g = np.asarray(g.cpu() if hasattr(g, 'cpu') else g)
                    gx = np.concatenate([g[b['x']] for b in layout['bodies']]).reshape(-1, 3)
                    gv = np.concatenate([g[b['v']] for b in layout['bodies']]).reshape(-1, 3)
                te.add_obs_grad(f, gx, gv)
            else:
                g = np.asarray(g.cpu() if hasattr(g, 'cpu') else g)
                gx, gv = self._dense_obs_grad(g, sim.engine.dtype, layout)
                sim.engine.add_grad(f, gx=gx, gv=gv)
        for k, fs in enumerate(layout.get('fields', [])):
            if self._field_obs_on_device():
                if on_gpu:
                    import torch
                    G = g[fs['slice']].reshape(fs['shape']).to(torch.float32).contiguous()
                else:
                    G = np.asarray(g.cpu() if hasattr(g, 'cpu') else g)[fs['slice']].reshape(fs['shape'])
                te.add_field_obs_grad(f, k, G, device=True)
            else:
                te.add_field_obs_grad(f, k, np.asarray(g.cpu() if hasattr(g, 'cpu') else g)[fs['slice']].reshape(fs['shape']))
        if layout['agent']:
            if on_gpu and self._device_obs:
                import torch
                grads = [g[s].to(torch.float32).contiguous() for s in layout['agent']]
            else:
                g = np.asarray(g.cpu() if hasattr(g, 'cpu') else g)
                grads = [np.array(g[s]) for s in layout['agent']]
                if not sim.engine.elib.has_ext:                  # (the oracle ABI has no pose-adjoint entry: only a zero cotangent can be dropped)
                    grads = [gi if np.any(gi != 0) else None for gi in grads]
            te.agent.add_state_grad(f, grads)

    def action_bounds(self):
        """(lo[action_dim], hi[action_dim]): the range a closed-loop policy maps each action entry into.  Here action_range for every entry;
        an environment whose entries do not all have the same meaning (CirculationEnv: the jet's radius must stay positive) overrides it."""
        ad = self.taichi_env.agent.action_dim
        return np.full((ad,), float(self.action_range[0])), np.full((ad,), float(self.action_range[1]))

    def _get_reward(self):
        return self.taichi_env.get_step_loss()['reward']

    def step(self, action):
        action = np.asarray(action).clip(self.action_range[0], self.action_range[1])
        self.taichi_env.step(action)
        obs = self._get_obs()
        reward = self._get_reward()
        assert self.t <= self.horizon
        done = self.t == self.horizon
        if np.isnan(reward):
            reward, done = -1000, True
        info = dict()
        if self._diagnostics:
            rec = self._diagnostics_record()
            info.update(rec)
            if rec['n_nonfinite'] > 0:
                reward, done = -1000, True
        if self._contact_info:
            info['contact'] = self.taichi_env.contact_wrench()
        return obs, reward, done, info

    def _diagnostics_record(self):
        """what step() reports with enable_diagnostics() on: a dict with at least 'n_nonfinite'.  Here the particle frame's summary; an
        environment whose state is not its particles (CirculationEnv: the smoke field) overrides it."""
        rec = self.taichi_env.frame_summary()
        return {k: rec[k] for k in ('courant', 'kinetic', 'n_used', 'n_nonfinite')}

    @property
    def t(self):
        return self.taichi_env.t
