"""TaichiEnv -- the object the envs and the optimiser talk to: it owns the simulator and hands agent, bodies, statics, smoke
field and loss to it (interface of fluidlab/fluidengine/taichi_env.py).

The name is kept so code written against the reference imports it unchanged; there is no Taichi here (no ti.init,
taichi_env.py:12): the simulator drives the MI355X HIP engine.  The one renderer is the headless HIP particle renderer
(setup_renderer(type='HIP'), render('rgb_array')); the reference's windowed GGUI / GL renderers are outside this build."""
import numpy as np

from fluidlab_amd.configs.macros import DTYPE_NP
from fluidlab_amd.fluidengine import agents as _agents
from fluidlab_amd.fluidengine.bodies import Bodies
from fluidlab_amd.fluidengine.meshes import Statics
from fluidlab_amd.fluidengine.simulators import MPMSimulator, SmokeField
from fluidlab_amd.utils.config import CfgNode

_NO_AGENT = 'Environment has no agent to execute action.'


class TaichiEnv:
    def __init__(self, dim=3, quality=1, particle_density=1e6, max_substeps_local=50, max_substeps_global=100000,
                 horizon=100, ckpt_dest='disk', gravity=(0.0, -10.0, 0.0), engine_lib=None, device=0, dt=None):
        self.dim, self.horizon, self.ckpt_dest = dim, horizon, ckpt_dest
        self.particle_density, self.max_substeps_global = particle_density, max_substeps_global
        self.simulator = MPMSimulator(dim=dim, quality=quality, horizon=horizon, max_substeps_local=max_substeps_local,
                                      max_substeps_global=max_substeps_global, gravity=gravity, ckpt_dest=ckpt_dest,
                                      engine_lib=engine_lib, device=device, dt=dt)
        self.max_substeps_local = self.simulator.max_substeps_local          # None (whole trajectory resident) is resolved there
        self.statics = Statics()
        self.particle_bodies = Bodies(dim=dim, particle_density=particle_density, elib=self.simulator.engine_library, device=device)
        self.agent = self.loss = self.smoke_field = self.renderer = None
        self.t = 0
        print('===>  TaichiEnv created.')

    # ---- scene description (called by FluidEnv.build_env before build())
    def setup_agent(self, agent_cfg):
        """agent_cfg: {type, params?, effectors: [{type, params, mesh?, boundary}]} (envs/configs/agent_*.yaml)"""
        make_agent = getattr(_agents, agent_cfg.type)
        self.agent = make_agent(max_substeps_local=self.max_substeps_local, max_substeps_global=self.max_substeps_global,
                                max_action_steps_global=self.horizon, ckpt_dest=self.ckpt_dest, **agent_cfg.get('params', {}))
        for entry in agent_cfg.effectors:
            eff = CfgNode(entry)
            self.agent.add_effector(type=eff.type, params=dict(eff.params), mesh_cfg=eff.get('mesh', None), boundary_cfg=dict(eff.boundary))

    def setup_boundary(self, **kwargs):
        self.simulator.setup_boundary(**kwargs)

    def setup_smoke_field(self, **kwargs):
        self.smoke_field = SmokeField(dim=self.dim, ckpt_dest=self.ckpt_dest, **kwargs)          # taichi_env.py:95-100

    def setup_loss(self, loss_cls, **kwargs):
        self.loss = loss_cls(max_loss_steps=self.horizon, **kwargs)

    def setup_renderer(self, type='HIP', **kwargs):
        """type='HIP': the headless particle renderer (renderers/hip_renderer.py; HIP engine only).  Before build() the renderer is built with
        the scene; after build() at once.  The reference's 'GGUI' and 'GL' need a window system and are not here."""
        if type != 'HIP':
            raise NotImplementedError(f"renderer type {type!r}: only the headless 'HIP' renderer is in this build (SURVEY 2 #12-#13)")
        from fluidlab_amd.fluidengine.renderers import HIPRenderer
        self.renderer = HIPRenderer(**kwargs)
        if self.simulator.engine is not None:
            self._build_renderer()

    def _build_renderer(self):
        try:
            self.renderer.build(self.simulator, self.particles)
        except Exception:
            self.renderer = None
            raise

    def add_static(self, **kwargs):
        self.statics.add_static(**kwargs)

    def add_body(self, **kwargs):
        self.particle_bodies.add_body(**kwargs)

    def build(self):
        """simulator first (it creates the engine), then whoever registers with it: smoke field, agent, loss (taichi_env.py:108-134)"""
        self.particles = self.particle_bodies.get()
        self.has_particles = self.particles is not None
        self.n_particles = len(self.particles['x']) if self.has_particles else 0
        self.simulator.build(self.agent, self.smoke_field, self.statics, self.particles)
        for part, args in ((self.smoke_field, (self.simulator, self.agent)), (self.agent, (self.simulator,)), (self.loss, (self.simulator,))):
            if part is not None:
                part.build(*args)
        if self.renderer is not None:
            self._build_renderer()
        self.t = 0

    # ---- differentiation switches
    def reset_grad(self):
        for part in (self.simulator, self.agent, self.loss):
            if part is not None:
                part.reset_grad()

    def enable_grad(self):
        self.simulator.enable_grad()

    def enable_material_grad(self):
        self.simulator.enable_material_grad()

    def get_material_grad(self, by='particle'):
        """d loss / d (mu, lam, rho) of the backward pass so far: MPMSimulator.get_material_grad"""
        return self.simulator.get_material_grad(by)

    def disable_grad(self):
        self.simulator.disable_grad()

    @property
    def grad_enabled(self):
        return self.simulator.grad_enabled

    # ---- stepping
    def _as_action(self, action, exact=False):
        if action is None:
            return None
        assert self.agent is not None, _NO_AGENT
        if getattr(action, 'is_cuda', False):               # a closed-loop policy's action on the engine's GPU stays there
            return action.detach()
        if exact:                                           # the action in the engine's own precision (fp64 on the fp64 oracle) instead of DTYPE_NP
            return np.array(action).astype(self.simulator.engine.dtype)
        return np.array(action).astype(DTYPE_NP)

    def step(self, action=None, exact=False):
        self.simulator.step(action=self._as_action(action, exact))
        if self.loss:
            self.loss.step()
        self.t += 1

    def step_grad(self, action=None, exact=False):
        if self.loss:                                   # the loss of a step is differentiated before the step itself
            self.loss.step_grad()
        self.simulator.step_grad(action=self._as_action(action, exact))

    def apply_agent_action_p(self, action_p):
        assert self.agent is not None, _NO_AGENT
        self.agent.apply_action_p(action_p)

    def apply_agent_action_p_grad(self, action_p):
        assert self.agent is not None, _NO_AGENT
        self.agent.apply_action_p_grad(action_p)

    # ---- loss and state access
    def get_step_loss(self):
        assert self.loss is not None
        return self.loss.get_step_loss()

    def get_final_loss(self):
        assert self.loss is not None
        return self.loss.get_final_loss()

    def get_final_loss_grad(self):
        assert self.loss is not None
        self.loss.get_final_loss_grad()

    def get_state(self):
        return {'state': self.simulator.get_state(), 'grad_enabled': self.grad_enabled}

    def set_state(self, state, grad_enabled=False):
        """restart from `state` at substep 0 (taichi_env.py:203-215)"""
        self.t = 0
        self.simulator.cur_substep_global = 0
        self.simulator.set_state(0, state)
        (self.enable_grad if grad_enabled else self.disable_grad)()
        if self.loss:
            self.loss.reset()

    def get_state_RL(self):
        return self.simulator.get_state_RL()

    def set_obs_particles(self, ids):
        self.simulator.set_obs_particles(ids)

    def get_obs_RL(self):
        """get_state_RL() restricted to the observation list, gathered on the device: MPMSimulator.get_obs_RL"""
        return self.simulator.get_obs_RL()

    def add_obs_grad(self, f=None, gx=None, gv=None):
        """the cotangent of get_obs_RL()'s rows goes into the adjoint of frame f: MPMSimulator.add_obs_grad"""
        self.simulator.add_obs_grad(f, gx, gv)

    def frame_summary(self, f=None, by='frame'):
        """per-frame / per-body diagnostics reduced on the device: MPMSimulator.frame_summary"""
        return self.simulator.frame_summary(f, by)

    def smoke_summary(self, s=None):
        """diagnostics of the smoke field's frame s (default: the current one) reduced on the device: SmokeField.summary"""
        if self.smoke_field is None:
            raise RuntimeError('smoke_summary: the scene has no smoke field')
        return self.smoke_field.summary(s)

    def contact_wrench(self):
        """The force and torque the material put on every collider during the step just taken -- the six numbers of a force/torque sensor per
        tool, the load on every static.  One dict per collider, the effectors first, then the statics:
          kind 'effector' | 'static', index (the effector's or the static's own);
          force    minus the summed impulse of the step's valid substeps, divided by their number times dt;
          torque   the same from the angular impulses -- for an effector about its own position (each substep's value is first moved to the
                   effector's position of that substep, ang_impulse - ref x impulse), for a static about the world origin;
          coverage valid substeps / substeps: a substep whose grid the engine did not keep (MPMSimulator.contact_wrench) reports nothing,
                   and force and torque average over the others (zeros when there is none);
          n_contacts the particle- and node-level contacts counted over the valid substeps."""
        rec = self.simulator.contact_wrench()
        n, dt = rec.shape[0], float(self.simulator.dt)
        out = []
        for c in range(rec.shape[1]):
            r = rec[:, c]
            ok = r['valid'] != 0
            n_ok = int(ok.sum())
            eff = int(r['kind'][0]) == 0
            ang = r['ang_impulse'] - np.cross(r['ref'], r['impulse']) if eff else r['ang_impulse']
            scale = -1.0 / (n_ok * dt) if n_ok else 0.0
            n_eff = int((rec['kind'][0] == 0).sum())
            out.append(dict(kind='effector' if eff else 'static', index=c if eff else c - n_eff,
                            force=scale * r['impulse'][ok].sum(axis=0), torque=scale * ang[ok].sum(axis=0),
                            coverage=n_ok / n, n_contacts=int(r['n_particles'][ok].sum() + r['n_nodes'][ok].sum())))
        return out

    def nearest_in_cloud(self, f, cloud, sel=None, axis_mask=7):
        """frame f against a target cloud, searched on the device: MPMSimulator.nearest_in_cloud"""
        return self.simulator.nearest_in_cloud(f, cloud, sel, axis_mask)

    def density_field(self, f=None, field=None, mat=None):
        """the density of frame f on a field, rasterised on the device: MPMSimulator.density_field"""
        return self.simulator.density_field(f, field, mat)

    def set_field_obs(self, fields):
        """the observation fields, a list of (DensityField, Sel, channels): MPMSimulator.set_field_obs"""
        self.simulator.set_field_obs(fields)

    def field_obs(self, f=None, k=0, device=False):
        """observation field k of frame f, [channels, n0, n1, n2] (density, momentum x y z): MPMSimulator.field_obs"""
        return self.simulator.field_obs(f, k, device)

    def add_field_obs_grad(self, f=None, k=0, G=None, device=False):
        """the cotangent of field_obs goes into the adjoint of frame f: MPMSimulator.add_field_obs_grad"""
        self.simulator.add_field_obs_grad(f, k, G, device)

    def enable_device_loss(self):
        """the task loss runs in the engine from here on (loss-term program): HostLoss.enable_device_loss.  After build(); HIP engine only."""
        if not hasattr(self.loss, 'enable_device_loss'):
            raise RuntimeError(f'{type(self.loss).__name__} has no loss-term program')
        self.loss.enable_device_loss()

    def enable_scene_render(self, **kwargs):
        """the pictures show the colliders and the smoke field from here on: HIPRenderer.enable_scene.  After build(); needs a renderer."""
        assert self.renderer is not None, 'No renderer available.'
        self.renderer.enable_scene(**kwargs)

    def enable_liquid_surface(self, **kwargs):
        """the pictures show the liquids as one smoothed, translucent surface from here on: HIPRenderer.enable_liquid_surface.  After build();
        needs a renderer.  Off by default."""
        assert self.renderer is not None, 'No renderer available.'
        self.renderer.enable_liquid_surface(**kwargs)

    def render_surface_buffers(self, tgt_particles=None):
        """(z_raw, z_smooth, thickness) of the liquid layer of the current frame: HIPRenderer.render_surface_buffers"""
        assert self.renderer is not None, 'No renderer available.'
        return self.renderer.render_surface_buffers(self.simulator.cur_substep_local, tgt_particles)

    def render(self, mode='human', tgt_particles=None):
        """mode='rgb_array': uint8 [H, W, 3] of the simulator's current frame (taichi_env.py:136-141); there is no window for 'human'"""
        assert self.renderer is not None, 'No renderer available.'
        if mode != 'rgb_array':
            raise NotImplementedError(f"render(mode={mode!r}): the renderer is headless, only 'rgb_array' is available")
        return self.renderer.render_frame(self.simulator.cur_substep_local, tgt_particles)

    def render_dev(self, tgt_particles=None):
        """the RGBA image of the current frame as a torch uint8 tensor [H, W, 4] on the engine's GPU, without a host copy"""
        assert self.renderer is not None, 'No renderer available.'
        return self.renderer.render_dev(self.simulator.cur_substep_local, tgt_particles)

    def render_buffers(self, tgt_particles=None):
        """(rgb, depth, id) of the current frame: HIPRenderer.render_buffers"""
        assert self.renderer is not None, 'No renderer available.'
        return self.renderer.render_buffers(self.simulator.cur_substep_local, tgt_particles)
